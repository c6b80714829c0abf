// rau_ctx.hip -- the rau_ctx object and the C ABI of include/rau.h.
//
// Orchestrates one training step of the Recurrent Answering Unit on one
// MI355X: question encoder (word embedding + 2-layer LSTM over <=T tokens),
// H weight-shared answering hops (attention over the S-position feature map,
// attention LSTM, classifier, cross-entropy) and the full backward pass into
// the three flat gradient buffers.  Reference being replaced: feval in
// experiments/Ours_SS/LstmAttCtrlGradNoiseDontSelect.lua:428-596 and the graph
// it drives (SS:198-316, model/ATTLSTM.lua, model/DeepLSTM.lua).
//
// Restructuring relative to the reference's module-by-module execution (all of
// it value-preserving; see DESIGN.md "Schedule"):
//   * work that does not depend on the recurrence is hoisted out of the loops
//     and batched: layer input projections over all tokens, the q projection
//     over all hops, dq = sum_h over hops, and every Linear weight gradient
//     (one [H*B]- or [T*B]-row GEMM per weight instead of one per clone);
//   * dropout masks are bit-packed and applied while staging GEMM operands;
//   * the dead gradient w.r.t. the feature map (SS:579 discards it) is skipped.
#include "rau_ctx.h"

static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

static int prof_collect(rau_ctx* ctx) {
  if (ctx->precs.empty()) return 0;
  HIPC(hipStreamSynchronize(ctx->st));
  HIPC(hipStreamSynchronize(ctx->st2));
  HIPC(hipStreamSynchronize(ctx->st3));
  if (ctx->stc) HIPC(hipStreamSynchronize(ctx->stc));   // the bank gather of a slot upload is bracketed there
  FILE* tl = nullptr;   // RAU_PROF_TIMELINE=path: per-launch (class, stream, start, end) in ms
  if (const char* p = std::getenv("RAU_PROF_TIMELINE")) tl = std::fopen(p, "a");
  for (auto& r : ctx->precs) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, r.a, r.b);
    if (tl) {
      float t0 = 0.f;
      hipEventElapsedTime(&t0, ctx->precs[0].a, r.a);
      std::fprintf(tl, "%s,%d,%.4f,%.4f\n", ctx->pcls[r.cls].name.c_str(), r.sid, t0, t0 + ms);
    }
    ctx->pcls[r.cls].ms += ms;
    ctx->evpool.push_back(r.a);
    ctx->evpool.push_back(r.b);
  }
  ctx->precs.clear();
  if (tl) { std::fprintf(tl, "#\n"); std::fclose(tl); }
  return 0;
}
// The Linear weight-gradient problems of the mult group (over hop-major rows) and of the encoder
// (over token-major rows): dW += dY^T X, db += column sums of dY.  dz and a are pitched (leading
// dimension = position pitch, Linear size = logical S).
static int mult_wgrad_problems(rau_ctx* ctx, TnProblem* pr) {
  const rau_config& c = ctx->cfg;
  const int S = ctx->Sp, SL = c.S, M = c.M, A = c.A, R = c.R, Q = ctx->Q;
  const size_t BR_ = (size_t)c.B * R;
  const float* hprev = ctx->hh;            // h_{0..H-1}
  const float* hnew = ctx->hh + BR_;       // h_{1..H}
  struct WG { Lin* l; const float* dY; long ldy; const float* X; long ldx; };
  const WG wgs[] = {
      {&ctx->cls, ctx->dl, ctx->Kp, ctx->mf, M},            {&ctx->lstm_out, ctx->dpre, M, hnew, R},
      {&ctx->lstm_i2h, ctx->dg4, 4 * R, ctx->j, M},    {&ctx->lstm_h2h, ctx->dg4, 4 * R, hprev, R},
      {&ctx->feat_attprob, ctx->dj, M, ctx->a, S},     {&ctx->att_mem, ctx->dz, S, hprev, R},
      {&ctx->att_q, ctx->du, A, ctx->qf, M},           {&ctx->q_proj, ctx->dqt, M, ctx->qd, Q},
      {&ctx->h_proj, ctx->dqt, M, hprev, R}};
  int n = 0;
  for (const WG& w : wgs) {
    const int out = w.l == &ctx->att_mem ? SL : w.l->out;
    const int in = w.l == &ctx->feat_attprob ? SL : w.l->in;
    pr[n++] = TnProblem{out, in, w.dY, w.ldy, w.X, w.ldx, w.l->dW, w.l->db};
  }
  return n;
}
static int enc_wgrad_problems(rau_ctx* ctx, size_t row0, TnProblem* pr) {
  struct WG { Lin* l; const float* dY; const float* X; };
  const WG wgs[] = {{&ctx->i2h[0], ctx->dG1, ctx->we}, {&ctx->h2h[0], ctx->dG1, ctx->h1},
                    {&ctx->i2h[1], ctx->dG2, ctx->x2}, {&ctx->h2h[1], ctx->dG2, ctx->h2}};
  int n = 0;
  for (const WG& w : wgs)
    pr[n++] = TnProblem{w.l->out, w.l->in, w.dY + row0 * w.l->out, w.l->out,
                        w.X + row0 * w.l->in, w.l->in, w.l->dW, w.l->db};
  return n;
}

// ---- everything the batch size decides beyond the tensor shapes ---------------------------------
// rau_create (for the capacity) and rau_set_batch_size (for the new size) both take it from here, so a
// resized context launches what a context created at that size launches and cannot drift from it.
struct BatchPlan {
  std::vector<int> groups;                   // forward hop-group partition (rau_ctx::groups)
  bool att_split, enc_ws, enc_ws_train;
  size_t ws[3], att_part;                    // workspace needs, floats: ws in the order of stream_ws()
  size_t mcount[5];                          // mask sites, elements
};
// the attention family of a B-sample batch (measurements: plan_batch below)
static bool att_family_split(const Policy& pol, int B) { return pol.att_split || (B <= 64 && !pol.att_fused); }
static void plan_batch(rau_ctx* ctx, int B, BatchPlan* p) {
  const rau_config& c = ctx->cfg;
  const int T = c.T, E = c.E, Rq = c.Rq, D = c.D, S = ctx->Sp, SL = c.S, M = c.M, A = c.A, R = c.R, K = c.K,
            H = c.H, Q = ctx->Q;
  // Default partition: pairs, then the last two hops alone.  The forward phase ends one hop after
  // the last group's GEMMs and the backward bulk work can start one hop into the backward chain
  // (measured on H = 8: 2,2,2,1,1 vs 2,2,2,2); pairs elsewhere keep the launches large.
  // RAU_HOP_GROUPS="4,2,1,1" overrides (sizes must sum to H).
  p->groups = hop_partition(ctx->policy.hop_groups, H);
  if (p->groups.empty()) {
    std::vector<int> sizes;
    if (B <= 64) {
      // small batches are bound by the recurrence's launches, not by the conv GEMMs: one group
      // (B = 32 / 64: 3.64 / 4.43 -> 3.55 / 4.33 ms; B = 128: 6.09 -> 6.49, so not there)
      sizes.push_back(H);
    } else {
      int left = H;
      while (left > 3) { sizes.push_back(2); left -= 2; }
      while (left > 0) { sizes.push_back(1); left -= 1; }
      if (H == 2) sizes = {1, 1};
    }
    p->groups = hop_partition(sizes, H);
  }
  p->mcount[RAU_MASK_WE] = (size_t)T * B * E;
  p->mcount[RAU_MASK_RNN] = (size_t)T * B * Rq;
  p->mcount[RAU_MASK_Q] = (size_t)H * B * Q;
  // one mask per hop clone, or (RAU_XDROP_TIED) one for all of them: hop 0's elements of the same stream
  p->mcount[RAU_MASK_X] = (size_t)(ctx->xdrop == RAU_XDROP_TIED ? 1 : H) * B * D * SL;
  p->mcount[RAU_MASK_MF] = (size_t)H * B * M;
  p->att_part = att_split_part_floats(B, S);
  // Same-box A/B (B=256, D=512, ms/step): fused 16-wave attention + split-K encoder 10.54-10.59,
  // split attention + fused encoder step 10.92-10.95, round-1 library 10.75-10.82.  The split
  // attention kernels and the fused LSTM step are faster ALONE (no bulk GEMM beside them): the
  // evaluate-mode forward uses the fused LSTM step; RAU_ATT_SPLIT forces the split attention kernels.
  // Small batches (one 16-wave workgroup per sample leaves most CUs idle): B = 32 / 64 / 128 fused
  // 3.83 / 4.57 / 6.06 ms, split in 8 row chunks 3.63 / 4.39 / 6.05 ms -> split up to B = 64
  // (RAU_ATT_FUSED keeps the fused kernels).
  p->att_split = att_family_split(ctx->policy, B);
  {
    // Weight-stationary persistent encoder (enc_ws.hip): chosen by shape, never by the environment in
    // normal use -- contexts of up to 64 samples (the strong-scaling shards of configs[3]) are bound
    // by the recurrence's launches.  RAU_ENC_WS=0|1 is the A/B override.
    const int e = ctx->policy.enc_ws;
    // measured in the step (MS weights, same box): B = 16 / 32 / 64 -> 3.00 / 3.49 / 4.46 ms with it,
    // 3.16 / 3.52 / 4.26 without; evaluate-mode forward 14.3 / 26.8 / 45.9 k vs 10.8 / 20.8 / 40.4 k QA/s.
    // Every workgroup reads all h rows of its sample half each step, so the traffic grows with B while
    // the weights it avoids re-reading do not: training contexts up to 32 samples, inference up to 64.
    // Its workgroups wait on each other's progress counters, so the whole grid must be resident at
    // once: asked of THIS device (a CPX partition or a reduced-CU device says no and keeps the
    // launch-per-step path).  If a bounded wait still gives up at run time (several contexts
    // competing for the CUs), persist_check() below turns the path off for the ctx -- for good: what
    // gave up was the device's residency, not the size, so a later rau_set_batch_size keeps it off.
    const bool fits = !ctx->persist_gave_up && enc_ws_ok(B, Rq) && enc_ws_fits_device(B);
    p->enc_ws_train = fits && (e >= 0 ? e != 0 : B <= 32);
    p->enc_ws = fits && (e >= 0 ? e != 0 : B <= 64);
  }
  {
    // split-K workspaces: one per stream (the two streams run concurrently)
    size_t sl2 = std::max(conv_wgrad_slab_floats(H * B, A, M, S),
                          conv_wgrad_slab_floats(H * B, M, D, S));
    if (ctx->bf16) sl2 = std::max(sl2, wgrad16_slab_floats(conv_mode(ctx), H * B, M, D, S));
    // The grouped Linear weight-gradient GEMMs' partial slabs.  They run on the weight-gradient stream or,
    // where the bulk stream is the longer path, at the END of the bulk stream (rau_backward), and take the
    // workspace of the stream they run on (StreamWs, rau_ctx.h): two launches that share a workspace must be
    // ordered by their stream.  (Round 4 first moved the mult group's GEMM to the bulk stream with the third
    // stream's slab still in its hands while the encoder group's GEMM used that slab on the third stream: the
    // two ran concurrently and overwrote each other's partials; tests/test_gpu_att_variants.py caught it.)
    size_t grp_floats = 0;
    {
      TnProblem pr[13];   // (only the shapes are read here)
      int n = mult_wgrad_problems(ctx, pr);
      for (int hh = 1; hh <= H; ++hh)
        grp_floats = std::max(grp_floats, gemm_tn_group_slab_floats(pr, n, hh * B));
      n = enc_wgrad_problems(ctx, 0, pr);
      for (int tt = 1; tt <= T; ++tt)
        grp_floats = std::max(grp_floats, gemm_tn_group_slab_floats(pr, n, tt * B));
    }
    p->ws[1] = std::max(sl2, grp_floats);
    const int rowsH = H * B, rowsT = T * B;
    const int shapes[][3] = {{K, M, rowsH},      {M, R, rowsH},      {4 * R, M, rowsH},
                             {4 * R, R, rowsH},  {M, S, rowsH},      {S, R, rowsH},
                             {A, M, rowsH},      {M, Q, rowsH},      {4 * Rq, E, rowsT},
                             {4 * Rq, Rq, rowsT}};
    // skinny split-K partials: every deferred GEMM of the hop loop must fit un-split in its share of
    // the slab (a quarter to a sixth), whatever its output width (4R, 4Rq, K, Q, M, A or S)
    size_t sl = (size_t)16 * B * std::max({4 * R, 4 * Rq, K, Q, M, A, S});
    for (auto& sh : shapes) sl = std::max(sl, gemm_tn_slab_floats(sh[0], sh[1], sh[2]));
    // a multiple of 16 floats: the quarter shares the hop chain carves out of it (hop_backward's regions) then start
    // on 16-byte boundaries, which state_grad_finish's quad loads of hop 0's partials rely on
    p->ws[0] = (sl + 15) & ~(size_t)15;
    // the weight-gradient stream's workspace also holds the grouped launches' partial slabs
    p->ws[2] = std::max(sl, grp_floats);
  }
}
// the launch decisions of `p` become the context's (the workspaces are the caller's business)
static void adopt_plan(rau_ctx* ctx, const BatchPlan& p) {
  ctx->groups = p.groups;
  for (int i = 0; i < 5; ++i) ctx->mcount[i] = p.mcount[i];
  ctx->att_split = p.att_split;
  ctx->enc_ws = p.enc_ws;
  ctx->enc_ws_train = p.enc_ws_train;
  for (int i = 0; i < 3; ++i) stream_ws(ctx)[i]->floats = p.ws[i];
}

// ================================================================== C ABI
extern "C" {

const char* rau_last_error(void) { return g_err; }
int rau_abi_version(void) { return RAU_ABI_VERSION; }

// ---- diagnostics: host-side predicates, no device touched (include/rau.h, last section)
int rau_split_guard_check(size_t ws_floats, size_t offset, int nsplit, size_t per_split_floats) {
  // a stand-in workspace in host memory: the check is pointer arithmetic only, nothing is dereferenced
  static thread_local float anchor[1];
  const float* base = anchor;
  split_ws_register(base, ws_floats);
  const bool ok = split_span_ok(base + offset, nsplit, per_split_floats);
  split_ws_unregister(base);
  if (!ok)
    return fail(RAU_ERR_STATE, "split-K partials [%zu + %d x %zu) outside a workspace of %zu floats: "
                               "nothing would be launched", offset, nsplit, per_split_floats, ws_floats);
  return RAU_OK;
}
int rau_enc_ws_coresident(int batch, int blocks_per_cu, int n_cus) {
  return (enc_ws_ok(batch, 512) && enc_ws_coresident(batch, blocks_per_cu, n_cus)) ? 1 : 0;
}

void rau_default_config(rau_config* cfg) {
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->B = 100;   // opt.batch_size default, SS:48
  cfg->T = 26;
  cfg->V = 14000;
  cfg->E = 200;
  cfg->Rq = 512;
  cfg->D = 512;
  cfg->S = 196;
  cfg->M = 512;
  cfg->A = 256;
  cfg->R = 512;
  cfg->K = 1000;
  cfg->H = 8;
  cfg->p_we = cfg->p_rnn = cfg->p_q = cfg->p_x = cfg->p_mf = 0.5f;
  cfg->dtype = RAU_F32;
  cfg->device_id = 0;
}

int rau_create(const rau_config* cfg, rau_ctx** out) {
  NEED(cfg && out, "rau_create: null argument");
  const rau_config& c = *cfg;
  NEED(c.B > 0 && c.T > 0 && c.V > 1 && c.H > 0, "rau_create: B,T,H must be > 0 and V > 1");
  NEED(c.E > 0 && c.E % 4 == 0, "rau_create: E=%d must be a positive multiple of 4", c.E);
  NEED(c.S > 0, "rau_create: S=%d must be positive", c.S);
  NEED(c.K >= 2, "rau_create: K=%d: a classification problem has at least two answers", c.K);
  NEED(c.Rq > 0 && c.Rq % 4 == 0 && c.R > 0 && c.R % 4 == 0 && c.M > 0 && c.M % 4 == 0 &&
           c.A > 0 && c.A % 4 == 0 && c.D > 0 && c.D % 4 == 0,
       "rau_create: Rq,R,M,A,D must be positive multiples of 4");
  const Policy policy = policy_from_env();   // once: the context never looks at the environment again
  {
    // a context may shrink its batch (rau_set_batch_size), never grow it: the family of B samples is the narrower
    const bool split = att_family_split(policy, c.B);
    // (the forward at the wider of its training and evaluate-mode forms)
    const AttMode tr = att_mode(policy, c.dtype, false), ev = att_mode(policy, c.dtype, true);
    const int smax = att_max_pitch(split, c.A, std::max(tr.waves_fwd, ev.waves_fwd), tr.waves_bwd);
    NEED(c.S <= smax,   // (a multiple of 4: the same bound on the pitch)
         "rau_create: S=%d is above the %d positions at which the %s attention kernels' LDS request still fits "
         "the 64 KB of a launch (B=%d, A=%d)", c.S, smax, split ? "split" : "fused", c.B, c.A);
  }
  NEED(c.dtype == RAU_F32 || c.dtype == RAU_BF16 || c.dtype == RAU_F32S,
       "rau_create: dtype %d not supported", c.dtype);
  const float ps[5] = {c.p_we, c.p_rnn, c.p_q, c.p_x, c.p_mf};
  for (float p : ps) NEED(p >= 0.f && p < 1.f, "rau_create: dropout p=%f out of [0,1)", p);

  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(RAU_ERR_DEVICE, "no HIP device available (%s); librau has no CPU fallback",
                hipGetErrorString(e));
  NEED(c.device_id >= 0 && c.device_id < ndev, "rau_create: device_id %d of %d", c.device_id, ndev);
  HIPC(hipSetDevice(c.device_id));
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, c.device_id));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(RAU_ERR_DEVICE, "device %d is %s; librau is built for gfx950 only", c.device_id,
                prop.gcnArchName);

  rau_ctx* ctx = new rau_ctx();
  ctx->cfg = c;
  ctx->policy = policy;
  ctx->Q = 4 * c.Rq;
  ctx->Sp = (c.S + 3) & ~3;
  ctx->Kp = (c.K + 3) & ~3;
  ctx->bf16 = c.dtype;   // 0 exact f32, 1 bf16-rounded operands, 2 split operands (conv GEMMs)
  // The device Philox masks keep an element when an 8-bit draw >= round(p * 256) (fill_masks): the
  // effective drop probability is p quantised to 1/256, and the inverted-dropout scale 1/(1-p)
  // uses THAT value so that E[mask * scale] = 1 exactly (the reference's 0.5 is representable).
  for (int i = 0; i < 5; ++i) {
    const float pq = std::lround(ps[i] * 256.0f) / 256.0f;
    if (pq >= 1.f) {
      delete ctx;
      return fail(RAU_ERR_INVALID, "rau_create: dropout p=%f rounds to 1 at 1/256 resolution", ps[i]);
    }
    ctx->mp[i] = pq;
    ctx->mp_exact[i] = ps[i];
  }
  *out = nullptr;
#define CK(x)                \
  do {                       \
    int rc_ = (x);           \
    if (rc_ != 0) {          \
      rau_destroy(ctx);      \
      return rc_;            \
    }                        \
  } while (0)
  {
    // the chain stream outranks the bulk stream: its short kernels are the critical
    // path and must not queue behind the bulk GEMMs' workgroups
    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    hipError_t es = hipStreamCreateWithPriority(&ctx->st, hipStreamNonBlocking, prio_hi);
    if (es == hipSuccess) es = hipStreamCreateWithPriority(&ctx->st2, hipStreamNonBlocking, prio_lo);
    if (es != hipSuccess) {
      delete ctx;
      return fail(RAU_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(es));
    }
  }
  hipEventCreate(&ctx->ev0);
  hipEventCreate(&ctx->ev1);
  const unsigned evflags = hipEventDisableTiming;
  for (hipEvent_t* e : {&ctx->evA, &ctx->evD, &ctx->evW, &ctx->evE, &ctx->evW3, &ctx->evM3, &ctx->evEnd, &ctx->evE1,
                        &ctx->evG0, &ctx->evG, &ctx->evQ0, &ctx->evQ, &ctx->evDq})
    hipEventCreateWithFlags(e, evflags);
  for (hipEvent_t& e : ctx->evGc) hipEventCreateWithFlags(&e, evflags);
  {
    int plo = 0, phi = 0;
    hipDeviceGetStreamPriorityRange(&plo, &phi);
    hipStreamCreateWithPriority(&ctx->st3, hipStreamNonBlocking, plo);
  }
  const hipStream_t owners[3] = {ctx->st, ctx->st2, ctx->st3};
  for (int i = 0; i < 3; ++i) stream_ws(ctx)[i]->owner = owners[i];
  ctx->cap = c.B;
  ctx->bgroups = hop_partition(policy.bwd_groups, c.H);
  ctx->evF.resize(c.H);
  ctx->evK.resize(c.H);

  ctx->evH.resize(c.H);
  for (int i = 0; i < c.H; ++i) {
    hipEventCreateWithFlags(&ctx->evF[i], evflags);
    hipEventCreateWithFlags(&ctx->evK[i], evflags);

    hipEventCreateWithFlags(&ctx->evH[i], evflags);
  }
  hipEventCreateWithFlags(&ctx->evHd, evflags);

  // S below is the position PITCH of the device tensors; SL the logical number of positions
  // (they differ only for maps like 7x7 = 49 -> 52: pad columns carry zero features, zero
  // attention and zero gradients, see att_fwd_fused)
  const int B = c.B, T = c.T, E = c.E, Rq = c.Rq, D = c.D, S = ctx->Sp, SL = c.S, M = c.M, A = c.A,
            R = c.R, K = c.K, H = c.H, Q = ctx->Q;
  // ---- parameter layouts (weight [out,in] then bias [out])
  {
    Group& g = ctx->grp[RAU_GROUP_EMBED];
    g.layout.push_back({"word_embed.weight", 0, c.V, E});  // LookupTable, SS:204
    g.n = (size_t)c.V * E;
  }
  {
    LayoutBuilder lb{&ctx->grp[RAU_GROUP_RNN]};
    ctx->i2h[0] = lb.take("rnn.l1.i2h", 4 * Rq, E);   // DeepLSTM.lua:42
    ctx->h2h[0] = lb.take("rnn.l1.h2h", 4 * Rq, Rq);  // DeepLSTM.lua:43
    ctx->i2h[1] = lb.take("rnn.l2.i2h", 4 * Rq, Rq);
    ctx->h2h[1] = lb.take("rnn.l2.h2h", 4 * Rq, Rq);
    ctx->grp[RAU_GROUP_RNN].n = lb.off;
  }
  {
    LayoutBuilder lb{&ctx->grp[RAU_GROUP_MULT]};
    ctx->q_proj = lb.take("q_embed.q_proj", M, Q);          // SS:233
    ctx->h_proj = lb.take("q_embed.h_proj", M, R);          // SS:234
    ctx->i_embed = lb.take("i_embed.conv", M, D);           // SS:240
    ctx->att_q = lb.take("attbycontent.qfeatatt", A, M);    // SS:246
    ctx->att_i = lb.take("attbycontent.ifeatproj", A, M);   // SS:247
    ctx->att_score = lb.take("attbycontent.attscore", 1, A);  // SS:251
    ctx->att_mem = lb.take("attbymemory.linear", SL, R);     // SS:287
    ctx->feat_attprob = lb.take("classifier.feat_attprob", M, SL);  // SS:271
    ctx->lstm_i2h = lb.take("classifier.attlstm.i2h", 4 * R, M);   // ATTLSTM.lua:6
    ctx->lstm_h2h = lb.take("classifier.attlstm.h2h", 4 * R, R);   // ATTLSTM.lua:7
    ctx->lstm_out = lb.take("classifier.lstm_out", M, R);          // SS:279
    ctx->cls = lb.take("classifier.out_score", K, M);              // SS:280
    ctx->do_pred = lb.take("classifier.out_do_pred", 1, M);        // SS:281
    ctx->grp[RAU_GROUP_MULT].n = lb.off;
  }
  for (int gi = 0; gi < 3; ++gi) {
    CK(dalloc(ctx, &ctx->grp[gi].w, ctx->grp[gi].n + 4, false));
    CK(dalloc(ctx, &ctx->grp[gi].g, ctx->grp[gi].n + 4, false));
  }
  for (int L = 0; L < 2; ++L) {
    bind(ctx->i2h[L], ctx->grp[RAU_GROUP_RNN]);
    bind(ctx->h2h[L], ctx->grp[RAU_GROUP_RNN]);
  }
  Lin* ml[] = {&ctx->q_proj, &ctx->h_proj, &ctx->i_embed, &ctx->att_q, &ctx->att_i,
               &ctx->att_score, &ctx->att_mem, &ctx->feat_attprob, &ctx->lstm_i2h,
               &ctx->lstm_h2h, &ctx->lstm_out, &ctx->cls, &ctx->do_pred};
  for (Lin* l : ml) bind(*l, ctx->grp[RAU_GROUP_MULT]);

  // ---- launch policy and workspace sizes of this batch size
  BatchPlan plan;
  plan_batch(ctx, B, &plan);
  adopt_plan(ctx, plan);
  // ---- batch
  BatchSlot& s0 = ctx->slot[0];   // (slot 1 comes with the asynchronous path: rau_batch.hip)
  CK(dalloc(ctx, &s0.feats, (size_t)B * D * S));
  CK(dalloc(ctx, &s0.tokens, (size_t)T * B));
  CK(dalloc(ctx, &s0.lens_d, (size_t)B));
  CK(dalloc(ctx, &s0.labels_d, (size_t)B));
  CK(dalloc(ctx, &s0.utok, (size_t)T * B));
  CK(dalloc(ctx, &s0.ustart, (size_t)T * B + 1));
  CK(dalloc(ctx, &s0.upos, (size_t)T * B));
  // ---- masks (bit-packed, +1 word slack)
  for (int i = 0; i < 5; ++i) CK(dalloc(ctx, &ctx->mbits[i], (ctx->mcount[i] + 31) / 32 + 1));
  // ---- encoder
  const size_t TB = (size_t)T * B;
  CK(dalloc(ctx, &ctx->we, TB * E));
  CK(dalloc(ctx, &ctx->G1, TB * 4 * Rq));
  CK(dalloc(ctx, &ctx->G2, TB * 4 * Rq));
  CK(dalloc(ctx, &ctx->c1, (TB + B) * Rq));
  CK(dalloc(ctx, &ctx->h1, (TB + B) * Rq));
  CK(dalloc(ctx, &ctx->c2, (TB + B) * Rq));
  CK(dalloc(ctx, &ctx->h2, (TB + B) * Rq));
  CK(dalloc(ctx, &ctx->tc1, TB * Rq));
  CK(dalloc(ctx, &ctx->tc2, TB * Rq));
  CK(dalloc(ctx, &ctx->x2, TB * Rq));
  CK(dalloc(ctx, &ctx->q, (size_t)B * Q));
  // ---- RAU
  const size_t HB = (size_t)H * B;
  CK(dalloc(ctx, &ctx->qd, HB * Q));
  CK(dalloc(ctx, &ctx->Yq, HB * M));
  CK(dalloc(ctx, &ctx->qf, HB * M));
  CK(dalloc(ctx, &ctx->xd, HB * D * S));
  // bf16 mode on maps the fused-dZ backward handles (the only backward that reads the bf16 form)
  if (ctx->bf16 == 1 && ctx->Sp == c.S && conv_dz_fused_ok(conv_mode(ctx), S, M) && !policy.xd_f32) {
    float* x16 = nullptr;
    CK(dalloc(ctx, &x16, (HB * D * S + 1) / 2));
    ctx->xd16 = x16;
    float *w16 = nullptr, *p16 = nullptr;
    CK(dalloc(ctx, &w16, ((size_t)M * D + 1) / 2));
    CK(dalloc(ctx, &p16, ((size_t)A * M + 1) / 2));
    ctx->WiT16 = w16;
    ctx->WpT16 = p16;
    if (dgrad16_ok(M, A, S, M) && att_bwd_dma_ok(att_mode(ctx), M, A, S)) {
      float* d16 = nullptr;
      CK(dalloc(ctx, &d16, (HB * A * S + 1) / 2));
      ctx->dS16 = d16;
    }
  }
  CK(dalloc(ctx, &ctx->I, HB * M * S));
  CK(dalloc(ctx, &ctx->T, HB * A * S));
  CK(dalloc(ctx, &ctx->u, HB * A));   // finished u = qf Wa^T + ba per hop (the backward's tanh(P + u))
  CK(dalloc(ctx, &ctx->P0, (size_t)B * A * S));
  CK(dalloc(ctx, &ctx->WiT, (size_t)M * D));
  CK(dalloc(ctx, &ctx->WpT, (size_t)A * M));
  CK(dalloc(ctx, &ctx->zm, (size_t)B * S));
  CK(dalloc(ctx, &ctx->att_part, plan.att_part));
  {
    float* f = nullptr;
    CK(dalloc(ctx, &f, 16));
    ctx->ws_cnt = reinterpret_cast<unsigned*>(f);
  }
  {
    float* f = nullptr;
    CK(dalloc(ctx, &f, 4));   // device error word of the persistent encoder (a bounded spin gave up)
    ctx->perr_d = reinterpret_cast<int*>(f);
    if (hipHostMalloc(reinterpret_cast<void**>(&ctx->perr_h), sizeof(int), hipHostMallocDefault) != hipSuccess)
      ctx->perr_h = nullptr;
    else
      *ctx->perr_h = 0;
  }
  CK(dalloc(ctx, &ctx->a, HB * S));
  CK(dalloc(ctx, &ctx->jv, (size_t)B * M));
  CK(dalloc(ctx, &ctx->j, HB * M));
  CK(dalloc(ctx, &ctx->g4, HB * 4 * R));
  CK(dalloc(ctx, &ctx->cc, (HB + B) * R));
  CK(dalloc(ctx, &ctx->hh, (HB + B) * R));
  CK(dalloc(ctx, &ctx->tc, HB * R));
  CK(dalloc(ctx, &ctx->mf, HB * M));
  CK(dalloc(ctx, &ctx->logits, HB * ctx->Kp));   // rows at the answer pitch, +0 in the pad
  CK(dalloc(ctx, &ctx->dl, HB * ctx->Kp));
  CK(dalloc(ctx, &ctx->lossrow, HB));
  CK(dalloc(ctx, &ctx->dopred, HB));
  CK(dalloc(ctx, &ctx->losses_d, (size_t)H));
  CK(dalloc(ctx, &ctx->hopw_d, HopwLayout(H).size));
  {  // ctx-owned pinned staging for the hop weights: the async upload never reads caller memory
    hipError_t eh = hipHostMalloc((void**)&ctx->hopw_h, 2 * HopwLayout(H).size * sizeof(float), hipHostMallocDefault);
    if (eh != hipSuccess) {
      rau_destroy(ctx);
      return fail(RAU_ERR_NOMEM, "hipHostMalloc(hop weights): %s", hipGetErrorString(eh));
    }
  }
  CK(dalloc(ctx, &ctx->argmax_d, HB));
  // ---- backward
  CK(dalloc(ctx, &ctx->dpre, HB * M));
  CK(dalloc(ctx, &ctx->dhn, HB * R));   // dpre Wo for all hops
  CK(dalloc(ctx, &ctx->dg4, HB * 4 * R));
  for (int i = 0; i < 2; ++i) {
    CK(dalloc(ctx, &ctx->dcn[i], (size_t)B * R));
    CK(dalloc(ctx, &ctx->dhp[i], (size_t)B * R));
  }
  CK(dalloc(ctx, &ctx->dj, HB * M));
  CK(dalloc(ctx, &ctx->da_lin, (size_t)B * S));
  CK(dalloc(ctx, &ctx->dz, HB * S));
  CK(dalloc(ctx, &ctx->du, HB * A));
  CK(dalloc(ctx, &ctx->dwsp, HB * A));
  CK(dalloc(ctx, &ctx->dZ, HB * M * S));
  CK(dalloc(ctx, &ctx->dqt, HB * M));
  CK(dalloc(ctx, &ctx->dQD, HB * Q));
  CK(dalloc(ctx, &ctx->dq, (size_t)B * Q));
  for (StreamWs* w : stream_ws(ctx)) {
    // split-K workspaces: one per stream (plan_batch); every consumer of K-split partials checks the span it is
    // about to read against these (split_guard.hip)
    CK(dalloc(ctx, &w->slab, w->floats));
    w->alloc = w->floats;
    split_ws_register(w->slab, w->floats);
  }
  {
    const int widest = std::max({4 * R, 4 * Rq, K, M, S, A, Q});
    CK(dalloc(ctx, &ctx->ws_side.coltmp, (size_t)32 * widest));
    CK(dalloc(ctx, &ctx->ws_bulk.coltmp, (size_t)32 * widest));
    CK(dalloc(ctx, &ctx->dbi_part, (size_t)H * B * M));       // per-sample row sums of dZ
    CK(dalloc(ctx, &ctx->tmpS, (size_t)S));
  }
  CK(dalloc(ctx, &ctx->dG1, TB * 4 * Rq));
  CK(dalloc(ctx, &ctx->dG2, TB * 4 * Rq));
  CK(dalloc(ctx, &ctx->dwe, TB * E));
  for (int L = 0; L < 2; ++L) {
    CK(dalloc(ctx, &ctx->edc[L][0], (size_t)B * Rq));
    CK(dalloc(ctx, &ctx->edc[L][1], (size_t)B * Rq));
  }
  CK(dalloc(ctx, &ctx->dkey, (size_t)2, false));   // (seed, step) outlive a resize
  CK(dalloc(ctx, &ctx->npart, (size_t)1024));
  CK(dalloc(ctx, &ctx->norms_d, (size_t)4));
  CK(dalloc(ctx, &ctx->upd_part, (size_t)3 * kUpdParts));
#undef CK
  {
    hipError_t es = hipStreamSynchronize(ctx->st);
    if (es != hipSuccess) {
      rau_destroy(ctx);
      return fail(RAU_ERR_DEVICE, "rau_create sync: %s", hipGetErrorString(es));
    }
  }
  *out = ctx;
  return RAU_OK;
}

void rau_destroy(rau_ctx* ctx) {
  if (!ctx) return;
  rau_comm_destroy(ctx);
  if (ctx->st_comm) hipStreamDestroy(ctx->st_comm);
  if (ctx->evC) hipEventDestroy(ctx->evC);
  if (ctx->st) hipStreamSynchronize(ctx->st);
  if (ctx->st2) hipStreamSynchronize(ctx->st2);
  if (ctx->st3) hipStreamSynchronize(ctx->st3);
  for (auto& g : ctx->graphs) hipGraphExecDestroy(g.exec);
  ctx->graphs.clear();   // rau_bank_destroy below drops the bank batches' graphs: not a second time
  for (StreamWs* w : stream_ws(ctx)) split_ws_unregister(w->slab);
  rau_bank_destroy(ctx);
  for (void* p : ctx->allocs) hipFree(p);
  if (ctx->hopw_h) hipHostFree(ctx->hopw_h);
  for (auto& r : ctx->precs) {
    hipEventDestroy(r.a);
    hipEventDestroy(r.b);
  }
  for (auto e : ctx->evpool) hipEventDestroy(e);
  if (ctx->ev0) hipEventDestroy(ctx->ev0);
  if (ctx->ev1) hipEventDestroy(ctx->ev1);
  for (hipEvent_t e : {ctx->evA, ctx->evD, ctx->evW, ctx->evE, ctx->evW3, ctx->evM3, ctx->evEnd, ctx->evE1,
                       ctx->evG0, ctx->evG, ctx->evQ0, ctx->evQ, ctx->evDq})
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : ctx->evGc)
    if (e) hipEventDestroy(e);
  if (ctx->st3) hipStreamDestroy(ctx->st3);
  if (ctx->perr_h) hipHostFree(ctx->perr_h);
  if (ctx->stc) { hipStreamSynchronize(ctx->stc); hipStreamDestroy(ctx->stc); }
  for (BatchSlot& s : ctx->slot) {
    if (s.feats_h) hipHostFree(s.feats_h);
    if (s.image_of_h) hipHostFree(s.image_of_h);
    if (s.bank_idx_h) hipHostFree(s.bank_idx_h);
    if (s.ans_h) hipHostFree(s.ans_h);
    if (s.nreg_h) hipHostFree(s.nreg_h);
    if (s.sw_h) hipHostFree(s.sw_h);
    if (s.cand_h) hipHostFree(s.cand_h);
    if (s.att_t_h) hipHostFree(s.att_t_h);
    if (s.pk_meta_h) hipHostFree(s.pk_meta_h);
    if (s.uploaded) hipEventDestroy(s.uploaded);
    if (s.consumed) hipEventDestroy(s.consumed);
  }
  for (hipEvent_t e : ctx->hopw_ev) if (e) hipEventDestroy(e);
  for (hipEvent_t e : ctx->bdev_ev) if (e) hipEventDestroy(e);
  for (int32_t* p : ctx->bdev_h) if (p) hipHostFree(p);
  for (hipEvent_t e : ctx->evF) hipEventDestroy(e);
  for (hipEvent_t e : ctx->evK) hipEventDestroy(e);

  for (hipEvent_t e : ctx->evH) hipEventDestroy(e);
  if (ctx->evHd) hipEventDestroy(ctx->evHd);
  if (ctx->st2) hipStreamDestroy(ctx->st2);
  if (ctx->st) hipStreamDestroy(ctx->st);
  delete ctx;
}

// ------------------------------------------------------------- parameters
static int check_group(rau_ctx* ctx, int group) {
  NEED(ctx, "null ctx");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  return 0;
}
int rau_params(rau_ctx* ctx, int group, float** weights, float** grads, size_t* n) {
  if (int rc = check_group(ctx, group)) return rc;
  if (weights) *weights = ctx->grp[group].w;
  if (grads) *grads = ctx->grp[group].g;
  if (n) *n = ctx->grp[group].n;
  return RAU_OK;
}
int rau_layout_count(const rau_ctx* ctx, int group) {
  if (!ctx || group < 0 || group > 2) return fail(RAU_ERR_INVALID, "bad ctx/group");
  return (int)ctx->grp[group].layout.size();
}
int rau_layout_entry(const rau_ctx* ctx, int group, int index, const char** name, size_t* offset,
                     int32_t* rows, int32_t* cols) {
  if (!ctx || group < 0 || group > 2) return fail(RAU_ERR_INVALID, "bad ctx/group");
  const auto& l = ctx->grp[group].layout;
  NEED(index >= 0 && index < (int)l.size(), "layout index %d out of range", index);
  if (name) *name = l[index].name.c_str();
  if (offset) *offset = l[index].off;
  if (rows) *rows = l[index].rows;
  if (cols) *cols = l[index].cols;
  return RAU_OK;
}
static int copy_group(rau_ctx* ctx, int group, bool grads, float* host, const float* chost,
                      size_t n) {
  if (int rc = check_group(ctx, group)) return rc;
  Group& g = ctx->grp[group];
  NEED(n == g.n, "group %d has %zu floats, caller passed %zu", group, g.n, n);
  float* dev = grads ? g.g : g.w;
  if (chost)
    HIPC(hipMemcpyAsync(dev, chost, n * sizeof(float), hipMemcpyHostToDevice, ctx->st));
  else
    HIPC(hipMemcpyAsync(host, dev, n * sizeof(float), hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return RAU_OK;
}
int rau_set_params(rau_ctx* ctx, int group, const float* host, size_t n) {
  NEED(host, "null host pointer");
  return copy_group(ctx, group, false, nullptr, host, n);
}
int rau_get_params(rau_ctx* ctx, int group, float* host, size_t n) {
  NEED(host, "null host pointer");
  return copy_group(ctx, group, false, host, nullptr, n);
}
int rau_get_grads(rau_ctx* ctx, int group, float* host, size_t n) {
  NEED(host, "null host pointer");
  return copy_group(ctx, group, true, host, nullptr, n);
}
int rau_set_grads(rau_ctx* ctx, int group, const float* host, size_t n) {
  NEED(host, "null host pointer");
  return copy_group(ctx, group, true, nullptr, host, n);
}
int rau_init_uniform(rau_ctx* ctx, uint64_t seed, float lo, float hi) {
  NEED(ctx, "null ctx");
  for (int gi = 0; gi < 3; ++gi)
    RUN("uniform_fill", 0, ctx->grp[gi].n * 4.0,
        uniform_fill(ctx->st, seed, (uint32_t)gi, ctx->grp[gi].n, lo, hi, ctx->grp[gi].w));
  return RAU_OK;
}
int rau_zero_grads(rau_ctx* ctx) {
  NEED(ctx, "null ctx");
  for (int gi = 0; gi < 3; ++gi)
    HIPC(hipMemsetAsync(ctx->grp[gi].g, 0, ctx->grp[gi].n * sizeof(float), ctx->st));
  return RAU_OK;
}

// ---------------------------------------------------------------- dropout
int rau_set_mode(rau_ctx* ctx, int mode) {
  NEED(ctx, "null ctx");
  NEED(mode == RAU_MODE_TRAIN || mode == RAU_MODE_EVAL, "bad mode %d", mode);
  ctx->mode = mode;
  return RAU_OK;
}
int rau_set_dropout_seed(rau_ctx* ctx, uint64_t seed, uint32_t step) {
  NEED(ctx, "null ctx");
  ctx->seed = seed;
  ctx->step = step;
  for (int i = 0; i < 5; ++i) ctx->mexplicit[i] = false;
  ctx->mod_masks_valid = false;
  // device copy for fill_masks (pageable source: staged at call time, ordered on the ctx stream)
  const uint64_t key[2] = {seed, (uint64_t)step};
  HIPC(hipMemcpyAsync(ctx->dkey, key, sizeof(key), hipMemcpyHostToDevice, ctx->st));
  return RAU_OK;
}
int rau_set_mask(rau_ctx* ctx, int site, const uint8_t* keep, size_t n) {
  NEED(ctx && keep, "null argument");
  NEED(site >= 0 && site < 5, "bad mask site %d", site);
  NEED(n == ctx->mcount[site], "mask site %d has %zu elements, caller passed %zu", site,
       ctx->mcount[site], n);
  std::vector<uint32_t> bits((n + 31) / 32, 0u);
  for (size_t i = 0; i < n; ++i)
    if (keep[i]) bits[i >> 5] |= 1u << (i & 31);
  HIPC(hipMemcpyAsync(ctx->mbits[site], bits.data(), bits.size() * 4, hipMemcpyHostToDevice,
                      ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  ctx->mexplicit[site] = true;
  ctx->mod_masks_valid = false;
  return RAU_OK;
}
// only: -1 = every site on the ctx stream; rau_forward fills the feature-map site (by far the largest,
// and read by the bulk stream only) on the bulk stream instead: skip = RAU_MASK_X, then only = RAU_MASK_X
static int gen_masks(rau_ctx* ctx, int skip = -1, int only = -1, hipStream_t stream = nullptr) {
  if (ctx->mode != RAU_MODE_TRAIN) return 0;
  hipStream_t s = stream ? stream : ctx->st;
  for (int i = 0; i < 5; ++i)
    if (i != skip && (only < 0 || i == only) && !ctx->mexplicit[i] && ctx->mp[i] > 0.f)
      RUNS(s, "fill_masks", 0, ctx->mcount[i] / 8.0,
           fill_masks(s, ctx->seed, (uint32_t)i, ctx->step, ctx->mp[i], ctx->mcount[i],
                      ctx->mbits[i], ctx->dkey));
  return 0;
}
int rau_get_mask(rau_ctx* ctx, int site, uint8_t* keep, size_t n) {
  NEED(ctx && keep, "null argument");
  NEED(site >= 0 && site < 5, "bad mask site %d", site);
  NEED(n == ctx->mcount[site], "mask site %d has %zu elements, caller passed %zu", site,
       ctx->mcount[site], n);
  if (!ctx->mexplicit[site]) {
    const int m = ctx->mode;
    ctx->mode = RAU_MODE_TRAIN;
    const int rc = gen_masks(ctx);
    ctx->mode = m;
    if (rc) return rc;
  }
  std::vector<uint32_t> bits((n + 31) / 32);
  HIPC(hipMemcpyAsync(bits.data(), ctx->mbits[site], bits.size() * 4, hipMemcpyDeviceToHost,
                      ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  for (size_t i = 0; i < n; ++i) keep[i] = (bits[i >> 5] >> (i & 31)) & 1u;
  return RAU_OK;
}

// ------------------------------------------------- feature-map dropout kind
// The forward reads ctx->xdrop (one masked map and the shared conv path in train mode), the backward what that
// forward recorded (fwd.tied), plan_batch the size of the mask site; nothing else depends on the kind.
int rau_set_feat_dropout(rau_ctx* ctx, int kind) {
  NEED(ctx, "null ctx");
  NEED(kind == RAU_XDROP_PER_HOP || kind == RAU_XDROP_TIED,
       "rau_set_feat_dropout: kind %d is neither RAU_XDROP_PER_HOP nor RAU_XDROP_TIED", kind);
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_feat_dropout: a step is being captured");
  if (kind == ctx->xdrop) return RAU_OK;
  // the hop sum of dS: allocated here, at the first use of the tied kind (never inside a captured step), for the
  // capacity, and cleared by rau_set_batch_size like every activation
  if (kind == RAU_XDROP_TIED && !ctx->dS_sum)
    if (int rc = dalloc(ctx, &ctx->dS_sum, (size_t)ctx->cap * ctx->cfg.A * ctx->Sp)) return rc;
  ctx->xdrop = kind;
  const rau_config& c = ctx->cfg;
  ctx->mcount[RAU_MASK_X] = (size_t)(kind == RAU_XDROP_TIED ? 1 : c.H) * c.B * c.D * c.S;
  ctx->mexplicit[RAU_MASK_X] = false;   // a caller's mask has the other kind's shape: back to the seeded stream
  ctx->mod_masks_valid = false;
  drop_forward(ctx);                    // the last forward is the other kind's: no backward without a new one
  return RAU_OK;
}
int rau_feat_dropout(rau_ctx* ctx, int* kind) {
  NEED(ctx && kind, "null argument");
  *kind = ctx->xdrop;
  return RAU_OK;
}

// ------------------------------------------------- feature-map gradient
// The backward reads ctx->feat_grad (group_conv_grads: one more block of launches per conv group on the bulk
// stream) and the graph key carries it.  Under RAU_FEAT_GRAD_IMAGES an image-table batch takes the per-image
// accumulate pass (xgrad_per_image: feat_grad_hops) and, in evaluate mode, the gathered forward (rau_forward).
int rau_set_feat_grad(rau_ctx* ctx, int on) {
  NEED(ctx, "null ctx");
  NEED(on == RAU_FEAT_GRAD_OFF || on == RAU_FEAT_GRAD_SAMPLES || on == RAU_FEAT_GRAD_IMAGES,
       "rau_set_feat_grad: mode %d is none of RAU_FEAT_GRAD_OFF, _SAMPLES, _IMAGES", on);
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_feat_grad: a step is being captured");
  if (on) {
    // for the capacity, at the first use (never inside a captured step); cleared by rau_set_batch_size like every
    // activation.  xg_tmp: one hop's product; xg_dz: one hop's dZ where the dgrad leaves dI (every map size outside
    // the 14 x 14 class, and the tied and evaluate-mode backward of any size: the mode may change after this call).
    // Each pointer on its own: a call that failed half way is completed by the next one, and the switch stays off
    // until all three exist.
    const rau_config& c = ctx->cfg;
    if (!ctx->xg_dX)
      if (int rc = dalloc(ctx, &ctx->xg_dX, (size_t)ctx->cap * c.D * ctx->Sp)) return rc;
    if (!ctx->xg_tmp)
      if (int rc = dalloc(ctx, &ctx->xg_tmp, (size_t)ctx->cap * c.D * ctx->Sp)) return rc;
    if (!ctx->xg_dz)
      if (int rc = dalloc(ctx, &ctx->xg_dz, (size_t)ctx->cap * c.M * ctx->Sp)) return rc;
  }
  // (a forward that ran under another mode stays differentiable or refused on its own record: fwd.table)
  if (on != ctx->feat_grad) ctx->bwd.dX = false;
  ctx->feat_grad = on;
  return RAU_OK;
}
int rau_feat_grad(rau_ctx* ctx, int* on) {
  NEED(ctx && on, "null argument");
  *on = ctx->feat_grad;
  return RAU_OK;
}
static int feat_grad_state(rau_ctx* ctx, const char* fn) {
  if (!ctx->feat_grad) return fail(RAU_ERR_STATE, "%s: the feature-map gradient is off (rau_set_feat_grad)", fn);
  if (!ctx->bwd.dX) return fail(RAU_ERR_STATE, "%s: no backward has run since the last forward", fn);
  return RAU_OK;
}
int rau_feat_grad_dev(rau_ctx* ctx, const float** dX, int32_t* pitch) {
  NEED(ctx, "null ctx");
  if (int rc = feat_grad_state(ctx, "rau_feat_grad_dev")) return rc;
  if (dX) *dX = ctx->xg_dX;
  if (pitch) *pitch = ctx->Sp;
  return RAU_OK;
}
int rau_feat_grad_rows(rau_ctx* ctx, int32_t* rows) {
  NEED(ctx && rows, "null argument");
  if (int rc = feat_grad_state(ctx, "rau_feat_grad_rows")) return rc;
  *rows = ctx->bwd.dX_rows;
  return RAU_OK;
}
int rau_get_feat_grad(rau_ctx* ctx, float* host) {
  NEED(ctx && host, "null argument");
  if (int rc = feat_grad_state(ctx, "rau_get_feat_grad")) return rc;
  const rau_config& c = ctx->cfg;
  HIPC(hipMemcpy2DAsync(host, (size_t)c.S * 4, ctx->xg_dX, (size_t)ctx->Sp * 4, (size_t)c.S * 4,
                        (size_t)ctx->bwd.dX_rows * c.D,
                        hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);
}

// ------------------------------------------------- feature-map normalisation
// The forward reads ctx->xnorm (feature_maps: one l2norm_features launch in front of everything that reads the maps,
// which then see an f32 batch), the backward too (one l2norm_backward behind the feature-map gradient); the graph key
// carries the kind and the bits of eps.  Nothing else depends on the switch.
int rau_set_feat_norm(rau_ctx* ctx, int kind, float eps) {
  NEED(ctx, "null ctx");
  NEED(kind == RAU_XNORM_NONE || kind == RAU_XNORM_L2,
       "rau_set_feat_norm: kind %d is neither RAU_XNORM_NONE nor RAU_XNORM_L2", kind);
  NEED(std::isfinite(eps) && eps > 0.f, "rau_set_feat_norm: eps = %g must be finite and > 0", (double)eps);
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_feat_norm: a step is being captured");
  if (kind == ctx->xnorm && (eps == ctx->xnorm_eps || kind == RAU_XNORM_NONE)) {
    ctx->xnorm_eps = eps;   // (off and off: only the value rau_feat_norm reports moves)
    return RAU_OK;
  }
  if (kind != RAU_XNORM_NONE) {
    // for the capacity, at the first use (never inside a captured step); cleared by rau_set_batch_size like every
    // activation.  Each pointer on its own: a call that failed half way is completed by the next one, and the
    // switch stays as it was until both exist.
    const rau_config& c = ctx->cfg;
    if (!ctx->xn)
      if (int rc = dalloc(ctx, &ctx->xn, (size_t)ctx->cap * c.D * ctx->Sp)) return rc;
    if (!ctx->nrm)
      if (int rc = dalloc(ctx, &ctx->nrm, (size_t)ctx->cap * ctx->Sp)) return rc;
  }
  ctx->xnorm = kind;
  ctx->xnorm_eps = eps;
  ctx->fwd.xn_rows = 0;
  ctx->bwd.dX = false;
  drop_forward(ctx);       // the last forward read other maps: no backward, no statistics, no outputs without
  ctx->mg.valid = false;   // a new forward
  return RAU_OK;
}
int rau_feat_norm(rau_ctx* ctx, int* kind, float* eps) {
  NEED(ctx, "null ctx");
  if (kind) *kind = ctx->xnorm;
  if (eps) *eps = ctx->xnorm_eps;
  return RAU_OK;
}
static int feat_norm_state(rau_ctx* ctx, const char* fn) {
  if (!ctx->xnorm) return fail(RAU_ERR_STATE, "%s: the normalisation is off (rau_set_feat_norm)", fn);
  if (!ctx->fwd.xn_rows) return fail(RAU_ERR_STATE, "%s: no forward has run since the switch was set", fn);
  return RAU_OK;
}
int rau_norm_feats_dev(rau_ctx* ctx, const float** xn, const float** nrm, int32_t* pitch, int32_t* rows) {
  NEED(ctx, "null ctx");
  if (int rc = feat_norm_state(ctx, "rau_norm_feats_dev")) return rc;
  if (xn) *xn = ctx->xn;
  if (nrm) *nrm = ctx->nrm;
  if (pitch) *pitch = ctx->Sp;
  if (rows) *rows = ctx->fwd.xn_rows;
  return RAU_OK;
}
int rau_get_norm_feats(rau_ctx* ctx, float* xn_host, float* nrm_host) {
  NEED(ctx, "null ctx");
  if (int rc = feat_norm_state(ctx, "rau_get_norm_feats")) return rc;
  const rau_config& c = ctx->cfg;
  const size_t rows = (size_t)ctx->fwd.xn_rows;
  if (xn_host)
    HIPC(hipMemcpy2DAsync(xn_host, (size_t)c.S * 4, ctx->xn, (size_t)ctx->Sp * 4, (size_t)c.S * 4, rows * c.D,
                          hipMemcpyDeviceToHost, ctx->st));
  if (nrm_host)
    HIPC(hipMemcpy2DAsync(nrm_host, (size_t)c.S * 4, ctx->nrm, (size_t)ctx->Sp * 4, (size_t)c.S * 4, rows,
                          hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);
}

// ------------------------------------------------------ answer criterion
// The forward's head reads ctx->answer_loss through step_truth(); the merged-hops record carries the kind of the
// forward it describes (MergeState::truth), the graph key the kind a step was captured under.  Nothing is allocated
// and nothing else depends on the kind.
int rau_set_answer_loss(rau_ctx* ctx, int kind) {
  NEED(ctx, "null ctx");
  NEED(kind == RAU_LOSS_CE || kind == RAU_LOSS_BCE,
       "rau_set_answer_loss: kind %d is neither RAU_LOSS_CE nor RAU_LOSS_BCE", kind);
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_answer_loss: a step is being captured");
  if (kind == ctx->answer_loss) return RAU_OK;
  ctx->answer_loss = kind;
  drop_forward(ctx);       // dl and the loss rows are the other criterion's: no backward, no statistics without
  ctx->mg.valid = false;   // a new forward
  return RAU_OK;
}
int rau_answer_loss(rau_ctx* ctx, int* kind) {
  NEED(ctx && kind, "null argument");
  *kind = ctx->answer_loss;
  return RAU_OK;
}

// ------------------------------------------------------------- batch size
int rau_batch_size(rau_ctx* ctx, int32_t* n, int32_t* capacity) {
  NEED(ctx, "null ctx");
  if (n) *n = ctx->cfg.B;
  if (capacity) *capacity = ctx->cap;
  return RAU_OK;
}

// A split-K workspace the new size needs more of than is there (the needs are not monotonic in the batch size:
// the split counts are chosen per shape): a second allocation, swapped in once all of them have succeeded.
int rau_set_batch_size(rau_ctx* ctx, int32_t n) {
  NEED(ctx, "null ctx");
  NEED(n >= 1 && n <= ctx->cap, "rau_set_batch_size: n=%d out of [1,%d] (the B of rau_create)", n, ctx->cap);
  if (n == ctx->cfg.B) return RAU_OK;
  if (ctx->prof_on) return fail(RAU_ERR_STATE, "rau_set_batch_size: profiling must be off");
  BatchPlan plan;
  plan_batch(ctx, n, &plan);
  // ---- allocate first: a failure leaves the context at the old size
  const auto wss = stream_ws(ctx);
  float* fresh[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; ++i) {
    if (plan.ws[i] <= wss[i]->alloc) continue;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&fresh[i]), plan.ws[i] * sizeof(float));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      for (float* f : fresh)
        if (f) hipFree(f);
      return fail(RAU_ERR_NOMEM, "rau_set_batch_size: hipMalloc(%zu bytes of split-K workspace) failed: %s; the "
                  "context keeps %d samples", plan.ws[i] * sizeof(float), hipGetErrorString(e), ctx->cfg.B);
    }
  }
  // ---- nothing may still read or write what is about to change: all four streams drain (pending uploads of
  // the asynchronous path included: they are dropped)
  for (hipStream_t s : {ctx->stc, ctx->st3, ctx->st2, ctx->st})
    if (s) HIPC(hipStreamSynchronize(s));
  if (ctx->persist_used && ctx->perr_h && *ctx->perr_h) {
    // the persistent encoder gave up in a step nobody has synchronised on yet: the finding is kept (persist_check)
    ctx->persist_gave_up = true;
    plan.enc_ws = plan.enc_ws_train = false;
  }
  for (int i = 0; i < 3; ++i) {
    if (!fresh[i]) continue;
    // captured steps hold the old workspace's address: all of them go (they are recaptured on demand)
    for (auto& gr : ctx->graphs) hipGraphExecDestroy(gr.exec);
    ctx->graphs.clear();
    split_ws_unregister(wss[i]->slab);
    void* old = wss[i]->slab;
    hipFree(old);
    ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), old), ctx->allocs.end());
    ctx->scratch.erase(std::remove_if(ctx->scratch.begin(), ctx->scratch.end(),
                                      [&](const std::pair<void*, size_t>& r) { return r.first == old; }),
                       ctx->scratch.end());
    ctx->allocs.push_back(fresh[i]);
    ctx->scratch.push_back({fresh[i], plan.ws[i] * sizeof(float)});
    wss[i]->slab = fresh[i];
    wss[i]->alloc = plan.ws[i];
  }
  // ---- the switch: shapes, launch policy, and the fail-closed guard's picture of the workspaces (the spans a
  // context of n samples would have registered; the allocations behind them are at least that large)
  ctx->cfg.B = n;
  adopt_plan(ctx, plan);
  for (StreamWs* w : wss) split_ws_register(w->slab, w->floats);
  // ---- every layout is dense in n, so what the old size left behind now lies where the step counts on the zeros
  // of a fresh context (the initial-state rows of c1 / h1 / c2 / h2, the pad columns of 7x7 maps, workspaces whose
  // tails are read as zeros): all batch-dependent storage is cleared, which is what rau_create leaves
  for (const auto& r : ctx->scratch) HIPC(hipMemsetAsync(r.first, 0, r.second, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  // ---- host-side state of a fresh context: no batch, no uploads, seeded masks, no results
  for (int si = 0; si < 2; ++si) {
    ctx->slot[si].held = BatchDesc{};
    ctx->slot[si].upload_pending = ctx->slot[si].consumed_valid = ctx->slot[si].ans_pending = false;
    ctx->slot[si].reg_pending = ctx->slot[si].att_pending = ctx->slot[si].sw_pending = false;
    ctx->slot[si].cand_pending = false;
    ++ctx->slot_serial[si];
  }
  ctx->cur_slot = 0;
  ctx->x_valid = false;
  ctx->fwd = FwdRecord{};
  ctx->bwd = BwdRecord{};
  for (int i = 0; i < 5; ++i) ctx->mexplicit[i] = false;
  ctx->mod_masks_valid = false;
  ctx->mg.invalidate();
  ctx->persist_used = false;
  if (ctx->perr_h) *ctx->perr_h = 0;
  return RAU_OK;
}

}  // extern "C"

// ================================================================ one hop
// The recurrence-dependent half of one answering hop (SS:292-307 given this hop's I and
// P = Wp I + bp), in two parts:
//   hop_forward_chain -- what the NEXT hop has to wait for: q_embed's recurrent half, attention,
//     the attention LSTM (8 dependent launches; next_c / next_h land in c_out / h_out);
//   hop_forward_head  -- what nothing on the recurrence waits for: merge_feat, out_score,
//     out_do_pred and the criterion head (SS:277-283, 488, 518), batched over `nh` consecutive
//     hops ([nh*B] rows) on any stream with its own split-K workspace.
// rau_forward runs the heads on the weight-gradient stream (idle during the forward pass), so the
// hop-to-hop critical path is the chain alone; the module-level entry points run both on st.
int hop_forward_chain(rau_ctx* ctx, int h, const float* cp, const float* hp, float* c_out,
                      float* h_out, const float* Ih, const float* Pin, const int32_t* img, const int32_t* nreg,
                      const float* zadd) {
  const rau_config& c = ctx->cfg;
  const int B = c.B, S = ctx->Sp, SL = c.S, M = c.M, A = c.A, R = c.R;
  hipStream_t st = ctx->st;
  const size_t BM_ = (size_t)B * M, BS_ = (size_t)B * S, BR_ = (size_t)B * R;
  float* qf = ctx->qf + (size_t)h * BM_;
  float* ah = ctx->a + (size_t)h * BS_;
  float* jh = ctx->j + (size_t)h * BM_;
  float* g4 = ctx->g4 + (size_t)h * B * 4 * R;
  // Split-K partials of several of these GEMMs are summed by their CONSUMER kernel instead of a
  // reduce launch (each launch on this dependent chain costs 8-20 us next to the bulk GEMMs):
  // the slab is carved into four regions so that partials can stay alive side by side.
  const StreamWs& ws = ctx->ws_chain;
  const size_t reg = ws.floats / 4;
  float *slab_u = ws.slab + reg, *slab_t = ws.slab + 2 * reg;
  int ns_u = 0, ns_t = 0, ns_i = 0;
  size_t off[3];
  {  // the three Linears fed by h_prev alone -- q_embed's recurrent half (SS:234), attbymemory
     // (SS:287) and the attention LSTM's h2h (ATTLSTM.lua:7) -- in ONE launch
    const float* Wt[3] = {ctx->h_proj.W, ctx->att_mem.W, ctx->lstm_h2h.W};
    const int Nt[3] = {M, SL, 4 * R};
    RUN("small_gemm", gflop(B, M + SL + 4 * R, R), 0,
        gemm_nt_hetero_deferred(st, lin_mode(ctx), 3, B, R, hp, R, Wt, R, Nt, slab_t, reg + reg / 2, &ns_t, off));
  }
  float *slab_z = slab_t + off[1], *slab_g = slab_t + off[2];
  {  // qf = tanh(Yq + h_prev Wh^T): the q half (with both biases) was computed for all hops at once
    LinOpts o;
    o.addend = ctx->Yq + (ctx->fwd.yq_shared ? 0 : (size_t)h * BM_);
    o.add_rs = M;
    o.act = 1;
    RUN("lin_reduce", 0, 0, lin_reduce_epilogue(st, B, M, ns_t, slab_t + off[0], qf, M, o));
  }
  {  // attbycontent SS:244-252: u = qf Wa^T (+ ba inside att_fwd_fused)
    LinOpts o = lin_opts(ctx, ws);
    o.slab = slab_u; o.slab_floats = reg; o.defer_splits = &ns_u;
    RUN("small_gemm", gflop(B, A, M), 0, gemm_nt(st, B, A, M, qf, M, ctx->att_q.W, M, ctx->u, A, o));
  }
  const int ns_z = ns_t, ns_h = ns_t;
  // tanh(P+u), score, softmax, attention-weighted sum: one pass per sample
  {
    AttPartials ap;
    ap.u_ns = ns_u; ap.u_bias = ctx->att_q.b;
    ap.z_ns = ns_z; ap.z_bias = ctx->att_mem.b;
    ap.SL = SL;
    ap.u_out = ctx->u + (size_t)h * B * A;   // tanh(P + u) itself is not kept: 25 % less traffic here
    // evaluate mode: no conv tile is resident while the hops run (I and P are hoisted), so the 16-wave form
    // fits and streams a sample faster (B = 256: 124.2 -> 129.5 k QA/s); the training step keeps 8 (att_mode)
    const AttMode am = att_mode(ctx);
    ap.img = img;   // image table: Pin and Ih hold one tile per image, sample b reads row img[b]
    ap.nreg = nreg;   // region counts: per SAMPLE, also where the tiles are per image
    ap.zadd = zadd;   // the caller's attention bias: per SAMPLE like the counts
    // (the profile tells the fused family's two kernels apart: the LDS-DMA one keeps the family's name)
    const char* fused_cls = att_fwd_dma_ok(am, M, A, S, false) ? "att_fwd_fused" : "att_fwd_fused_regs";
    if (!ctx->att_split)
      RUN(fused_cls, 2.0 * B * S * (A + M), ((double)B * A * S + BM_ * S) * 4,
          att_fwd_fused(st, am, B, M, A, S, Pin, slab_u, ctx->att_score.W, ctx->att_score.b, slab_z, Ih, qf,
                        nullptr, ah, ctx->jv, ap));
    else
      RUN("att_fwd_split", 2.0 * B * S * (A + M), ((double)B * A * S + BM_ * S) * 4,
          att_fwd_split(st, am, B, M, A, S, Pin, slab_u, ctx->att_score.W, ctx->att_score.b, slab_z, Ih, qf,
                        ah, ctx->jv, ctx->att_part, ap));
  }
  {  // classifier SS:265-283
    LinOpts o = lin_opts(ctx, ws);
    o.slab_floats = reg;
    o.bias = ctx->feat_attprob.b;
    o.addend = ctx->jv;
    o.add_rs = M;
    RUN("small_gemm", gflop(B, M, SL), 0, gemm_nt(st, B, M, SL, ah, S, ctx->feat_attprob.W, SL, jh, M, o));
  }
  {  // j Wx^T partials right behind the recurrent ones; the cell kernel sums both + both biases
    LinOpts o = lin_opts(ctx, ws);
    o.slab = slab_g + (size_t)ns_h * B * 4 * R; o.slab_floats = reg / 2; o.defer_splits = &ns_i;
    RUN("small_gemm", gflop(B, 4 * R, M), 0,
        gemm_nt(st, B, 4 * R, M, jh, M, ctx->lstm_i2h.W, M, g4, 4 * R, o));
    LstmFwdCells cells{};
    cells.n = 1;
    LstmFwdCell& C = cells.c[0];
    C.g4 = g4; C.has_input = 0; C.b1 = ctx->lstm_i2h.b; C.b2 = ctx->lstm_h2h.b;
    C.slab = slab_g; C.nsplit = ns_h + ns_i;
    C.c_prev = cp; C.cp_rs = R; C.c = c_out; C.c_rs = R; C.h = h_out; C.h_rs = R;
    C.tanhc = ctx->tc + (size_t)h * BR_;
    C.drop_out = nullptr; C.mask = nullptr; C.mask_e0 = 0; C.mscale = 1.f;
    RUN("lstm_fwd", 0, BR_ * 4.0 * 10, lstm_fwd_multi(st, GATES_ATT, B, R, cells));
  }
  return RAU_OK;
}

// merge_feat = dropout(j + h' Wo^T + bo), logits = merge_feat Wc^T + bc, do_pred, cross-entropy +
// first-max argmax for hops [h0, h0 + nh): rows = nh * B.  h' rows are ctx->hh slots h0+1 .. (the
// chain's h_out); it runs on ws.owner and uses the first two quarters of that stream's split-K workspace.
int hop_forward_head(rau_ctx* ctx, const StreamWs& ws, int h0, int nh, const Truth& truth) {
  const rau_config& c = ctx->cfg;
  hipStream_t s = ws.owner;
  const size_t reg = ws.floats / 4;
  const int B = c.B, M = c.M, R = c.R, K = c.K, Kp = ctx->Kp;
  const Masks m = masks_of(ctx);
  const size_t BM_ = (size_t)B * M, BR_ = (size_t)B * R;
  const int rows = nh * B;
  const float* hnew = ctx->hh + (size_t)(h0 + 1) * BR_;
  const float* jh = ctx->j + (size_t)h0 * BM_;
  float* mfh = ctx->mf + (size_t)h0 * BM_;
  float* lg = ctx->logits + (size_t)h0 * B * Kp;
  int ns_c = 0;
  {
    LinOpts o = lin_opts(ctx, ws);
    o.slab_floats = reg;
    o.bias = ctx->lstm_out.b;
    o.addend = jh;
    o.add_rs = M;
    o.emask = m.mf; o.emask_e0 = (size_t)h0 * BM_; o.emscale = m.s_mf;
    RUNS(s, "head_gemm", gflop(rows, M, R), 0,
         gemm_nt(s, rows, M, R, hnew, R, ctx->lstm_out.W, R, mfh, M, o));
  }
  {  // out_score SS:280: partials finished (+ bias) by the criterion-head kernel
    LinOpts o = lin_opts(ctx, ws);
    o.slab = ws.slab + reg; o.slab_floats = reg; o.defer_splits = &ns_c;
    RUNS(s, "head_gemm", gflop(rows, K, M), 0,
         gemm_nt(s, rows, K, M, mfh, M, ctx->cls.W, M, lg, Kp, o));
  }
  RUNS(s, criterion_class(truth), 0, (double)rows * K * 12,
       criterion_head(s, rows, K, M, lg, truth, mfh, ctx->do_pred.W, ctx->do_pred.b, ctx->dl + (size_t)h0 * B * Kp,
                      ctx->lossrow + (size_t)h0 * B, ctx->argmax_d + (size_t)h0 * B, ctx->dopred + (size_t)h0 * B,
                      ws.slab + reg, ns_c, ctx->cls.b, lg, B, Kp));
  return RAU_OK;
}

int hop_forward(rau_ctx* ctx, int h, const float* cp, const float* hp, float* c_out, float* h_out,
                const float* Ih, const float* Pin, const Truth& truth, const int32_t* nreg, const float* zadd) {
  if (int rc = hop_forward_chain(ctx, h, cp, hp, c_out, h_out, Ih, Pin, nullptr, nreg, zadd)) return rc;
  if (h_out != ctx->hh + (size_t)(h + 1) * ctx->cfg.B * ctx->cfg.R)
    return fail(RAU_ERR_INVALID, "hop_forward: h_out must be the ctx's hop slot");
  return hop_forward_head(ctx, ctx->ws_chain, h, 1, truth);
}

// Backward of hop_forward (hand-derived, SURVEY 8a "exact backward of one hop"): from the
// gradients at {logits, next_c, next_h} to dpre, dg4, dj, dz, dS (in T), du, dq~ in the
// hop-h slots and {dc_prev, dh_prev}.  Weight gradients and the 1x1-conv gradients are formed
// by the callers from those slots.
//
// What is on the recurrence's critical path is kept to 10 dependent launches:
//   * dpre = (dl Wc) (.) mask and dhn = dpre Wo do not depend on the recurrence; the step-level
//     caller forms them for all hops at once up front (g.dpre_ready / g.dhn_all);
//   * the three contributions to dh_prev (dg Wr, dz Wm, dq~ Wh) stay K-split partials, laid out
//     back to back, and are summed by the NEXT hop's lstm_bwd (g.dh_part_*), so none of them
//     costs a reduce launch; dj Wf's partials are summed inside att_bwd_fused;
//   * dg Wx and dg Wr share their A operand: one batched launch when M == R.
int hop_backward(rau_ctx* ctx, int h, const float* cp, const float* Ih, const HopGrad& g) {
  const rau_config& c = ctx->cfg;
  const int B = c.B, S = ctx->Sp, SL = c.S, M = c.M, A = c.A, R = c.R, K = c.K;
  hipStream_t st = ctx->st;
  const Masks m = masks_of(ctx);
  const size_t BM_ = (size_t)B * M, BS_ = (size_t)B * S, BR_ = (size_t)B * R;
  const float* qf = ctx->qf + (size_t)h * BM_;
  float* Th = ctx->T + (size_t)h * B * A * S;   // becomes dS in place
  const float* ah = ctx->a + (size_t)h * BS_;
  const float* g4 = ctx->g4 + (size_t)h * B * 4 * R;
  float* dpre = ctx->dpre + (size_t)h * BM_;
  float* dg4 = ctx->dg4 + (size_t)h * B * 4 * R;
  float* djh = ctx->dj + (size_t)h * BM_;
  float* dzh = ctx->dz + (size_t)h * BS_;
  float* duh = ctx->du + (size_t)h * B * A;
  float* dqt = ctx->dqt + (size_t)h * BM_;
  float* dc_out = g.dc_out;
  // split-K workspace: region 0 = partials that are reduced right away (lin_opts' default) or
  // consumed by the next kernel; regions 1..3 = this hop's dj partials followed by the dh_prev
  // partials, which live until the next hop's lstm_bwd has read them
  const StreamWs& ws = ctx->ws_chain;
  const size_t reg = ws.floats / 4;
  float* X = ws.slab + reg;
  const size_t Xcap = 3 * reg;
  if (!g.dpre_ready) {
    {  // dmf = dlogits Wc ; dpre = dmf (.) mask   (do_pred grad is zero, SS:566)
      LinOpts o = lin_opts(ctx, ws);
      o.slab_floats = reg;
      o.addend = g.dmf_add;   // module-level callers: gradient through do_pred (zero in feval)
      o.add_rs = M;
      o.emask = m.mf; o.emask_e0 = (size_t)h * BM_; o.emscale = m.s_mf;
      RUN("small_gemm", gflop(B, M, K), 0,
          gemm_nn(st, B, M, K, g.dl, ctx->Kp, ctx->cls.W, M, dpre, M, o));
    }
    // dhn = dpre Wo + dh_next, the K-split partials of dpre Wo summed inside lstm_bwd
    int nsp = 0;
    LinOpts o = lin_opts(ctx, ws);
    o.slab_floats = reg;
    o.defer_splits = &nsp;
    RUN("small_gemm", gflop(B, R, M), 0, gemm_nn(st, B, R, M, dpre, M, ctx->lstm_out.W, R, ctx->dhn, R, o));
    RUN("lstm_bwd", 0, BR_ * 4.0 * 12,
        lstm_bwd(st, GATES_ATT, B, R, g4, cp, R, ctx->tc + (size_t)h * BR_, nullptr, R, g.dh_next,
                 g.dc_next, dg4, dc_out, nullptr, 0, nullptr, nullptr, 0, ws.slab, nsp));
  } else {
    // dhn rows of this hop + the previous hop_backward's dh_prev partials (+ dh_next if given)
    RUN("lstm_bwd", 0, BR_ * 4.0 * 12,
        lstm_bwd(st, GATES_ATT, B, R, g4, cp, R, ctx->tc + (size_t)h * BR_,
                 g.dhn_all + (size_t)h * BR_, R, g.dh_next, g.dc_next, dg4, dc_out, nullptr, 0,
                 nullptr, nullptr, 0, g.dh_part, g.dh_part_ns));
  }
  // dj partials = dg Wx ; dh_prev partials #1 = dg Wr
  int ns_j = 0, ns_h = 0;
  float* dhp = nullptr;      // start of this hop's dh_prev partials [ns_h][B][R]
  const bool dead = g.dh_prev_dead;
  if (M == R && !dead) {
    const float* Ap[2] = {dg4, dg4};
    const float* Wp[2] = {ctx->lstm_i2h.W, ctx->lstm_h2h.W};
    RUN("small_gemm", 2 * gflop(B, M, 4 * R), 0,
        gemm_nn_batched_deferred(st, lin_mode(ctx), 2, B, M, 4 * R, Ap, 4 * R, Wp, M, X, Xcap / 2, &ns_j));
    dhp = X + (size_t)ns_j * BM_;
    ns_h = ns_j;
  } else {
    LinOpts o1 = lin_opts(ctx, ws);
    o1.slab = X; o1.slab_floats = Xcap / 4; o1.defer_splits = &ns_j;
    RUN("small_gemm", gflop(B, M, 4 * R), 0,
        gemm_nn(st, B, M, 4 * R, dg4, 4 * R, ctx->lstm_i2h.W, M, djh, M, o1));
    dhp = X + (size_t)ns_j * BM_;
    if (!dead) {
      LinOpts o2 = lin_opts(ctx, ws);
      o2.slab = dhp; o2.slab_floats = Xcap / 4; o2.defer_splits = &ns_h;
      RUN("small_gemm", gflop(B, R, 4 * R), 0,
          gemm_nn(st, B, R, 4 * R, dg4, 4 * R, ctx->lstm_h2h.W, R, nullptr, R, o2));
    }
  }
  {  // dj = dpre + sum of partials
    LinOpts o;
    o.addend = dpre;
    o.add_rs = M;
    RUN("lin_reduce", 0, 0, lin_reduce_epilogue(st, B, M, ns_j, X, djh, M, o));
  }
  int ns_a = 0;
  {  // da = dj Wf  (+ attselect term and the gradient at the attprob OUTPUT inside att_bwd_fused)
    LinOpts o = lin_opts(ctx, ws);
    o.slab_floats = reg;
    o.defer_splits = &ns_a;
    RUN("small_gemm", gflop(B, SL, M), 0,
        gemm_nn(st, B, SL, M, djh, M, ctx->feat_attprob.W, SL, ctx->da_lin, S, o));
  }
  if (!ctx->att_split)
    RUN("att_bwd_fused", 2.0 * B * S * (A + M), ((double)B * A * S * 2 + BM_ * S) * 4,
        att_bwd_fused(st, att_mode(ctx), B, M, A, S, Ih, djh, ah, ws.slab, ctx->att_score.W, Th, dzh, duh,
                      ctx->dwsp + (size_t)h * B * A, ctx->fwd.I_shared ? ctx->P0 : Th,
                      ctx->u + (size_t)h * B * A, ns_a, SL, g.da_out,
                      g.ds16 ? (void*)((uint16_t*)ctx->dS16 + (size_t)h * B * A * S) : nullptr));
  else
    RUN("att_bwd_split", 2.0 * B * S * (A + M), ((double)B * A * S * 2 + BM_ * S) * 4,
        att_bwd_split(st, att_mode(ctx), B, M, A, S, Ih, djh, ah, ws.slab, ctx->att_score.W, Th, dzh, duh,
                      ctx->dwsp + (size_t)h * B * A, ctx->fwd.I_shared ? ctx->P0 : Th,
                      ctx->u + (size_t)h * B * A, ctx->att_part, ns_a, SL, g.da_out));
  if (g.ev_conv_ready) HIPC(hipEventRecord(g.ev_conv_ready, st));
  const size_t used = (size_t)(dhp - X);
  if (!dead) {  // dh_prev partials #2 = dz Wm
    int ns = 0;
    LinOpts o = lin_opts(ctx, ws);
    o.slab = dhp + (size_t)ns_h * BR_;
    o.slab_floats = (Xcap - used) / 3;
    o.defer_splits = &ns;
    RUN("small_gemm", gflop(B, R, SL), 0, gemm_nn(st, B, R, SL, dzh, S, ctx->att_mem.W, R, nullptr, R, o));
    ns_h += ns;
  }
  {  // dq~ = (dj + du Wa) (1 - qf^2)
    LinOpts o = lin_opts(ctx, ws);
    o.slab_floats = reg;
    o.addend = djh;
    o.add_rs = M;
    o.ymul = qf;
    o.y_rs = M;
    RUN("small_gemm", gflop(B, M, A), 0, gemm_nn(st, B, M, A, duh, A, ctx->att_q.W, M, dqt, M, o));
  }
  if (!dead) {  // dh_prev partials #3 = dq~ Wh
    int ns = 0;
    LinOpts o = lin_opts(ctx, ws);
    o.slab = dhp + (size_t)ns_h * BR_;
    o.slab_floats = (Xcap - used) / 3;
    o.defer_splits = &ns;
    RUN("small_gemm", gflop(B, R, M), 0, gemm_nn(st, B, R, M, dqt, M, ctx->h_proj.W, R, nullptr, R, o));
    ns_h += ns;
  }
  if (g.dh_part_out) {   // the next hop_backward's lstm_bwd sums them
    *g.dh_part_out = dead ? nullptr : dhp;
    *g.dh_part_ns_out = dead ? 0 : ns_h;
  } else {               // module-level callers want dh_prev itself
    LinOpts o;
    RUN("lin_reduce", 0, 0, lin_reduce_epilogue(st, B, R, ns_h, dhp, g.dh_out, R, o));
  }
  return RAU_OK;
}

// ================================================================ image side
// i_embed SS:238-242 and attbycontent's ifeatproj (SS:247-249), which is hop-invariant given I: P = Wp I + bp;
// the per-hop half (+u, tanh, score, softmax, context) is att_fwd_fused.
int image_forward(rau_ctx* ctx, hipStream_t s, int n, const void* x, bool x_is_b16, float* I, float* P) {
  const rau_config& c = ctx->cfg;
  const int D = c.D, S = ctx->Sp, M = c.M, A = c.A;
  const double nS = (double)n * S;
  if (x_is_b16) {
    RUNS(s, "conv_embed_fwd", gflop(M, nS, D), nS * D * 2 + nS * M * 4,
         conv_embed_fwd_b16(s, n, D, S, M, x, ctx->WiT16, ctx->i_embed.b, I));
    RUNS(s, "conv_att_pre", gflop(A, nS, M), (nS * M + nS * A) * 4,
         conv_att_pre_b16(s, n, M, S, A, I, ctx->WpT16, ctx->att_i.b, P));
  } else {
    RUNS(s, "conv_embed_fwd", gflop(M, nS, D), (nS * D + nS * M) * 4,
         conv_embed_fwd(s, conv_mode(ctx), n, D, S, M, (const float*)x, ctx->WiT, ctx->i_embed.b, I));
    RUNS(s, "conv_att_pre", gflop(A, nS, M), (nS * M + nS * A) * 4,
         conv_att_pre(s, conv_mode(ctx), n, M, S, A, I, ctx->WpT, ctx->att_i.b, P));
  }
  return RAU_OK;
}

// The 1x1-conv gradients of g.n maps on `s`, with the bulk stream's split-K workspace: the dgrad, then the two
// weight gradients (the att_i one is independent of dZ).  Where the per-sample tiling applies (g.dzf) the dgrad's
// epilogue also applies (1 - I^2) and hands back per-sample row sums (the i_embed bias gradient): the i_embed
// weight gradient then stages a plain operand (one global load and no VALU work per element less).
int conv_grads(rau_ctx* ctx, hipStream_t s, const ConvGrads& g) {
  const rau_config& c = ctx->cfg;
  const int n = g.n, D = c.D, S = ctx->Sp, M = c.M, A = c.A;
  const double nAS = (double)n * A * S, nMS = (double)n * M * S, nDS = (double)n * D * S;
  float* slab = ctx->ws_bulk.slab;
  const ConvMode cm = conv_mode(ctx);   // (light: contexts whose recurrence is the longer path, chain_bound)
  if (g.dzf)
    RUNS(s, "conv_att_dgrad", gflop(M, (double)n * S, A), (nAS + 3.0 * nMS) * 4,
         conv_att_dgrad_dz(s, cm, n, M, S, A, (const float*)g.dS, ctx->att_i.W, g.dj, g.a, g.I, (float*)g.dZ,
                           g.dbi_part, g.dz_is_b16 ? 1 : 0, g.ds_is_b16 ? 1 : 0));
  else
    RUNS(s, "conv_att_dgrad", gflop(M, (double)n * S, A), (nAS + 2.0 * nMS) * 4,
         conv_att_dgrad(s, cm, n, M, S, A, (const float*)g.dS, ctx->att_i.W, g.dj, g.a, (float*)g.dZ));
  if (g.tied_hops > 1)   // + dj_h (x) a_h of the other active hops (hop 0's came out of the dgrad's epilogue)
    RUNS(s, "outer_sum", 2.0 * (g.tied_hops - 1) * nMS,
         (2.0 * nMS + (double)(g.tied_hops - 1) * ((double)n * M + (double)n * S)) * 4,
         outer_sum(s, g.tied_hops, n, M, S, g.dj, g.a, (float*)g.dZ));
  if (g.ds_is_b16)
    RUNS(s, "conv_att_wgrad", gflop(A, M, (double)n * S), nAS * 2 + nMS * 4,
         conv_att_wgrad_ds16(s, n, M, S, A, (const uint16_t*)g.dS, g.I, ctx->att_i.dW, slab));
  else
    RUNS(s, "conv_att_wgrad", gflop(A, M, (double)n * S), (nAS + nMS) * 4,
         conv_att_wgrad(s, cm, n, M, S, A, (const float*)g.dS, g.I, ctx->att_i.dW, slab));
  if (g.x_is_b16)
    RUNS(s, "conv_embed_wgrad", gflop(M, D, (double)n * S), nMS * 2 + nDS * 2,
         conv_embed_wgrad_b16(s, cm, n, D, S, M, (const uint16_t*)g.dZ, (const uint16_t*)g.X, ctx->i_embed.dW, slab));
  else
    RUNS(s, "conv_embed_wgrad", gflop(M, D, (double)n * S), (nMS * (g.dzf ? 1 : 2) + nDS) * 4,
         conv_embed_wgrad(s, cm, n, D, S, M, (const float*)g.dZ, g.I, (const float*)g.X, ctx->i_embed.dW, slab,
                          ctx->i_embed.db, g.dzf));
  return RAU_OK;
}

extern "C" {

// ================================================================ forward
// The forward / backward seam (the bulk stream and the matrix pipes wait there for the chain).  Policy::seam
// (RAU_SEAM=<mask>, A/B; default 3): 1 = a train-mode forward with labels also forms the backward's two
// recurrence-free head products (dpre, dhn) behind each group's criterion head on the third stream;
// 2 = a group's conv gradients start behind att_bwd of its first hop instead of behind the hop's last launch.

// ---------------- encoder, SS:443-462
// Layer-1 cell t+1 and layer-2 cell t do not depend on each other, so the two layers
// advance as a wavefront: per step ONE batched split-K GEMM (h1 W_h2h1^T for layer 1;
// x2 W_i2h2^T and h2 W_h2h2^T for layer 2; same shapes) and ONE two-cell LSTM kernel
// that sums the partials -- TL+1 steps of 2 launches instead of 2*TL steps of 2.
static int encoder_forward(rau_ctx* ctx, const Masks& m) {
  const BatchSlot& bs = cur_batch(ctx);
  const rau_config& c = ctx->cfg;
  const int B = c.B, E = c.E, Rq = c.Rq, TL = bs.held.max_len;
  const size_t BRq = (size_t)B * Rq;
  hipStream_t st = ctx->st;
  if (TL > 0) {
    const int rows = TL * B;
    const size_t G4 = (size_t)B * 4 * Rq;
    RUN("embed_fwd", 0, rows * E * 8.0,
        embed_fwd(st, rows, E, c.V, ctx->grp[RAU_GROUP_EMBED].w, bs.tokens, m.we, m.s_we, ctx->we));
    const bool ws_path = (ctx->mode == RAU_MODE_EVAL ? ctx->enc_ws : ctx->enc_ws_train) && ctx->perr_h;
    // Layer-1 input projection of every token (no recurrence in it).  Only the first tokens' rows
    // are needed at once: they stay on this stream, the rest runs on the weight-gradient stream
    // (idle in the forward pass) and the wavefront waits for it where it first reads it.
    const int t_head = (!ws_path && side_split(ctx) && TL > kEncHeadTokens) ? kEncHeadTokens : TL;
    {
      LinOpts o = lin_opts(ctx, ctx->ws_chain);
      o.bias = ctx->i2h[0].b;
      o.bias2 = ctx->h2h[0].b;
      RUN("enc_i2h_gemm", gflop(t_head * B, 4 * Rq, E), 0,
          gemm_nt(st, t_head * B, 4 * Rq, E, ctx->we, E, ctx->i2h[0].W, E, ctx->G1, 4 * Rq, o));
    }
    if (t_head < TL) {
      HIPC(hipEventRecord(ctx->evG0, st));            // embed_fwd is done
      HIPC(hipStreamWaitEvent(ctx->st3, ctx->evG0, 0));
      LinOpts o = lin_opts(ctx, ctx->ws_side);
      o.bias = ctx->i2h[0].b;
      o.bias2 = ctx->h2h[0].b;
      // in chunks, so that the recurrence only ever waits for the rows it is about to read
      const int nchunk_env = ctx->policy.enc_chunks;   // RAU_ENC_CHUNKS
      const int nchunk = std::max(1, std::min(nchunk_env > 0 ? nchunk_env : kEncSideChunks,
                                              std::min(kEncSideChunks, TL - t_head)));
      const int per = (TL - t_head + nchunk - 1) / nchunk;
      for (int cch = 0; cch <= kEncSideChunks; ++cch) ctx->enc_chunk_tok[cch] = TL;
      for (int cch = 0, t0 = t_head; t0 < TL; ++cch, t0 += per) {
        const int nt = std::min(per, TL - t0), r1 = nt * B;
        ctx->enc_chunk_tok[cch] = t0;
        RUNS(ctx->st3, "enc_i2h_gemm", gflop(r1, 4 * Rq, E), 0,
             gemm_nt(ctx->st3, r1, 4 * Rq, E, ctx->we + (size_t)t0 * B * E, E, ctx->i2h[0].W, E,
                     ctx->G1 + (size_t)t0 * G4, 4 * Rq, o));
        HIPC(hipEventRecord(ctx->evGc[cch], ctx->st3));
      }
    }
    // the recurrence's wait in front of wavefront step s (layer-1 cell of token s, 1-based): the chunk that
    // starts with that token
    auto wait_i2h_rows = [&](int s) -> int {
      if (t_head >= TL) return 0;
      for (int cch = 0; cch < kEncSideChunks; ++cch)
        if (ctx->enc_chunk_tok[cch] == s - 1 && s - 1 < TL) HIPC(hipStreamWaitEvent(st, ctx->evGc[cch], 0));
      return 0;
    };
    if (ws_path) {
      // both layers, all tokens: one launch, weights resident in registers (enc_ws.hip)
      EncWsParams q{};
      q.B = B; q.R = Rq; q.TL = TL; q.bf16 = ctx->bf16 == 1;
      q.G1 = ctx->G1; q.G2 = ctx->G2; q.h1 = ctx->h1; q.c1 = ctx->c1; q.tc1 = ctx->tc1; q.x2 = ctx->x2;
      q.h2 = ctx->h2; q.c2 = ctx->c2; q.tc2 = ctx->tc2;
      q.Wh1 = ctx->h2h[0].W; q.Wi2 = ctx->i2h[1].W; q.Wh2 = ctx->h2h[1].W;
      q.bi2 = ctx->i2h[1].b; q.bh2 = ctx->h2h[1].b;
      q.mask = m.rnn; q.mscale = m.s_rnn;
      q.cnt = ctx->ws_cnt; q.err = ctx->perr_d;
      RUN("enc_ws", (double)TL * 3 * gflop(B, 4 * Rq, Rq), 0, enc_ws_forward(st, GATES_DEEP, q));
      HIPC(hipMemcpyAsync(ctx->perr_h, ctx->perr_d, sizeof(int), hipMemcpyDeviceToHost, st));
      ctx->persist_used = true;
    } else
    for (int s = 1; s <= TL + 1; ++s) {
      if (int rc = wait_i2h_rows(s)) return rc;   // G1 rows of token s
      const float* Ap[3];
      const float* Wp[3];
      int nb = 0, i0 = -1, i1 = -1, i2 = -1;
      if (s <= TL && s >= 2) { Ap[nb] = ctx->h1 + (size_t)(s - 1) * BRq; Wp[nb] = ctx->h2h[0].W; i0 = nb++; }
      if (s >= 2) { Ap[nb] = ctx->x2 + (size_t)(s - 2) * BRq; Wp[nb] = ctx->i2h[1].W; i1 = nb++; }
      if (s >= 3) { Ap[nb] = ctx->h2 + (size_t)(s - 2) * BRq; Wp[nb] = ctx->h2h[1].W; i2 = nb++; }
      int nsp = 0;
      if (nb > 0)
        RUN("enc_h2h_gemm", gflop(B, 4 * Rq, Rq) * nb, 0,
            gemm_nt_batched_deferred(st, lin_mode(ctx), nb, B, 4 * Rq, Rq, Ap, Rq, Wp, Rq, ctx->ws_chain.slab,
                                     ctx->ws_chain.floats, &nsp));
      LstmFwdCells cells{};
      if (s <= TL) {  // layer-1 cell t = s
        LstmFwdCell& C1 = cells.c[cells.n++];
        C1.g4 = ctx->G1 + (size_t)(s - 1) * G4;
        C1.has_input = 1;
        C1.slab = i0 >= 0 ? ctx->ws_chain.slab + (size_t)i0 * nsp * G4 : nullptr;
        C1.nsplit = i0 >= 0 ? nsp : 0;
        C1.c_prev = ctx->c1 + (size_t)(s - 1) * BRq; C1.cp_rs = Rq;
        C1.c = ctx->c1 + (size_t)s * BRq; C1.c_rs = Rq;
        C1.h = ctx->h1 + (size_t)s * BRq; C1.h_rs = Rq;
        C1.tanhc = ctx->tc1 + (size_t)(s - 1) * BRq;
        C1.drop_out = ctx->x2 + (size_t)(s - 1) * BRq;   // layer-2 input, DeepLSTM.lua:39
        C1.mask = m.rnn; C1.mask_e0 = (size_t)(s - 1) * BRq; C1.mscale = m.s_rnn;
      }
      if (s >= 2) {  // layer-2 cell t = s - 1
        const int t = s - 1;
        LstmFwdCell& C2 = cells.c[cells.n++];
        C2.g4 = ctx->G2 + (size_t)(t - 1) * G4;
        C2.has_input = 0;
        C2.b1 = ctx->i2h[1].b; C2.b2 = ctx->h2h[1].b;
        C2.slab = ctx->ws_chain.slab + (size_t)i1 * nsp * G4;      // x2 W_i2h2^T then h2 W_h2h2^T partials
        C2.nsplit = i2 >= 0 ? 2 * nsp : nsp;
        C2.c_prev = ctx->c2 + (size_t)(t - 1) * BRq; C2.cp_rs = Rq;
        C2.c = ctx->c2 + (size_t)t * BRq; C2.c_rs = Rq;
        C2.h = ctx->h2 + (size_t)t * BRq; C2.h_rs = Rq;
        C2.tanhc = ctx->tc2 + (size_t)(t - 1) * BRq;
        C2.drop_out = nullptr; C2.mask = nullptr; C2.mask_e0 = 0; C2.mscale = 1.f;
      }
      RUN("lstm_fwd", 0, BRq * 4.0 * 10 * cells.n, lstm_fwd_multi(st, GATES_DEEP, B, Rq, cells));
    }
  }
  return 0;
}

// The passes on `sb` that make the maps the convs read out of the batch's nX maps `feats`.  In train mode each hop
// clone has its own dropout mask on the feature map (SS:239, SS:343-347) -> xd[h] = X (.) mask_h (tied: one copy); in
// evaluate mode the convs read the batch itself.  Sets ctx->fwd.xw and ctx->fwd.x_shared; *x16_out: the hop copies are bf16.
static int feature_maps(rau_ctx* ctx, hipStream_t sb, const Masks& m, const float* feats, int nX, bool* x16_out) {
  const rau_config& c = ctx->cfg;
  const int B = c.B, D = c.D, S = ctx->Sp, SL = c.S, M = c.M, A = c.A, H = c.H;
  const bool tied = ctx->fwd.tied;
  // the batch's element type: 16-bit and fp8 maps are widened (exactly) by the pass that reads them
  int ft = cur_batch(ctx).held.feat_type;
  // rau_set_feat_norm: the nX maps are normalised per position first, and everything below -- dropout in its three
  // forms, the no-mask path, the weight gradients' x_shared -- runs on xn as on an f32 batch (no widen pass either)
  ctx->fwd.xn_rows = 0;
  if (ctx->xnorm) {
    RUNS(sb, "l2norm_features", 3.0 * nX * D * S, (double)nX * D * S * (feat_elem_bytes(ft) + 4),
         l2norm_features(sb, nX, D, SL, S, feats, ft, ctx->xnorm_eps, ctx->xn, ctx->nrm));
    feats = ctx->xn;
    ft = RAU_FEAT_F32;
    ctx->fwd.xn_rows = nX;
  }
  // feature-map dropout, SS:239: unless the caller supplied the mask, the pass that makes the H masked
  // copies draws the keep bits itself (they have no other reader on this path)
  // bf16 mode: the hop copies of the feature map are stored as bf16 (to halve an H-fold buffer; the one tied
  // copy stays f32 in xd and feeds the f32-storage kernels, which round their operands themselves)
  const bool x16 = m.x && ctx->xd16 && !tied;
  const int HX = tied ? 1 : H;         // masked copies: the mask site has HX * B * D * SL elements
  const bool x_gen = m.x && !ctx->mexplicit[RAU_MASK_X] && SL == S && ((size_t)B * D * S) % 16 == 0;
  ctx->fwd.xgen = x_gen;   // the bits never reach memory: a feature-map gradient regenerates them (xgrad.hip)
  ctx->fwd.seed = ctx->seed;
  ctx->fwd.step = ctx->step;
  if (!x_gen)
    if (int rc = gen_masks(ctx, -1, RAU_MASK_X, sb)) return rc;
  RUNS(sb, "transpose", 0, (double)M * D * 8, transpose2d(sb, M, D, ctx->i_embed.W, ctx->WiT, ctx->WiT16));
  RUNS(sb, "transpose", 0, (double)A * M * 8, transpose2d(sb, A, M, ctx->att_i.W, ctx->WpT, ctx->WpT16));
  const double xb = (double)feat_elem_bytes(ft);   // bytes per element read from the batch
  if (x_gen)
    RUNS(sb, "dropout_features", 0, (double)B * D * S * xb + (double)HX * B * D * S * (x16 ? 2 : 4),
         dropout_features_gen(sb, ctx->seed, RAU_MASK_X, ctx->step, ctx->mp[RAU_MASK_X], ctx->dkey, HX,
                              (size_t)B * D * S, feats, m.s_x, x16 ? (void*)ctx->xd16 : (void*)ctx->xd,
                              x16 ? 1 : 0, ft));
  else if (x16)
    RUNS(sb, "dropout_features", 0, (double)B * D * S * xb + (double)H * B * D * S * 2,
         dropout_features_b16(sb, H, (size_t)B * D * S, feats, m.x, m.s_x, ctx->xd16, ft));
  else if (m.x)
    RUNS(sb, "dropout_features", 0, (double)B * D * S * xb + (double)HX * B * D * S * 4,
         dropout_features(sb, HX, (size_t)B * D * S, feats, m.x, m.s_x, ctx->xd, 0, SL, S, ft));
  // no mask: the GEMMs read the batch itself -- a 16-bit one through its f32 image in xd (unused here),
  // so that they are the f32 batch's kernels with the f32 batch's operands
  ctx->fwd.xw = const_cast<float*>(feats);
  if (!m.x && ft != RAU_FEAT_F32) {
    ctx->fwd.xw = ctx->xd;
    RUNS(sb, "widen_features", 0, (double)nX * D * S * (xb + 4),
         widen_features(sb, (size_t)nX * D, SL, S, feats, ctx->fwd.xw, ft));
  }
  ctx->fwd.x_shared = m.x ? ctx->xd : ctx->fwd.xw;   // what the shared path's i_embed reads (and its weight gradient)
  *x16_out = x16;
  return RAU_OK;
}

// dpre = (dl Wc (+ addend)) (.) mask and dhn = dpre Wo of hops [h0, h0 + nh) on ws.owner: the backward's two
// products that do not depend on the recurrence.
static int head_dgrad(rau_ctx* ctx, const StreamWs& ws, int h0, int nh, const float* addend) {
  const rau_config& c = ctx->cfg;
  const int B = c.B, M = c.M, R = c.R, K = c.K;
  const size_t BM_ = (size_t)B * M, BR_ = (size_t)B * R;
  const Masks m = masks_of(ctx);
  hipStream_t s = ws.owner;
  LinOpts o = lin_opts(ctx, ws);
  if (addend) { o.addend = addend; o.add_rs = M; }
  o.emask = m.mf; o.emask_e0 = (size_t)h0 * BM_; o.emscale = m.s_mf;
  RUNS(s, "head_dgrad", gflop(nh * B, M, K), 0,
       gemm_nn(s, nh * B, M, K, ctx->dl + (size_t)h0 * B * ctx->Kp, ctx->Kp, ctx->cls.W, M,
               ctx->dpre + (size_t)h0 * BM_, M, o));
  const LinOpts o2 = lin_opts(ctx, ws);
  RUNS(s, "head_dgrad", gflop(nh * B, R, M), 0,
       gemm_nn(s, nh * B, R, M, ctx->dpre + (size_t)h0 * BM_, M, ctx->lstm_out.W, R, ctx->dhn + (size_t)h0 * BR_, R,
               o2));
  return RAU_OK;
}

// Classifier + criterion heads of the finished hops [gstart, h] on the side stream, head_max hops per launch
static int forward_heads(rau_ctx* ctx, int gstart, int h, int head_max, const Truth& truth, bool dpre) {
  for (int h0 = gstart; h0 <= h; h0 += head_max)
    if (int rc = hop_forward_head(ctx, ctx->ws_side, h0, std::min(head_max, h + 1 - h0), truth)) return rc;
  // The backward's first two products do not depend on the recurrence either: dpre = (dl Wc) (.) mask
  // and dhn = dpre Wo of these hops follow their criterion head on the same (idle) stream, so the
  // forward / backward seam -- where the bulk stream and the matrix pipes wait for the chain -- is two
  // GEMMs shorter.  dl is not yet scaled by the hop weights (they arrive with rau_backward); both
  // products are linear in it, so rau_backward scales dl, dpre and dhn together.
  if (dpre) return head_dgrad(ctx, ctx->ws_side, gstart, h + 1 - gstart, nullptr);
  return RAU_OK;
}

// rau_forward; bwd_forms_dpre: the backward of this (captured) step forms dpre / dhn itself (StepLoss::forms_dpre)
static int forward_impl(rau_ctx* ctx, bool bwd_forms_dpre) {
  NEED(ctx, "null ctx");
  BatchSlot& bs = cur_batch(ctx);
  if (!bs.held.have) return fail(RAU_ERR_STATE, "rau_forward: no batch (call rau_set_batch)");
  ctx->mg.valid = false;   // the hop outputs are being overwritten
  ctx->bwd.dX = ctx->bwd.dq = false;   // ... and the gradients at the maps and at an attached question another forward's
  ctx->bwd.dstate = false;             // ... and the one at an attached initial state
  ctx->bwd.dbias = false;              // ... and the one at an attached attention bias
  const rau_config& c = ctx->cfg;
  const int B = c.B, Rq = c.Rq, D = c.D, S = ctx->Sp, M = c.M, A = c.A, R = c.R, H = c.H, Q = ctx->Q;
  const int TL = bs.held.max_len;
  hipStream_t st = ctx->st;
  if (int rc = gen_masks(ctx, RAU_MASK_X)) return rc;
  const Masks m = masks_of(ctx);
  // RAU_XDROP_TIED: every hop clone sees the SAME masked map, so a train-mode step takes the shared path too (one
  // masked copy, both convs once) and its backward sums the hops in front of one set of conv gradients
  const bool tied = ctx->mode == RAU_MODE_TRAIN && ctx->xdrop == RAU_XDROP_TIED;
  ctx->fwd.I_shared = (m.x == nullptr) || tied;
  ctx->fwd.tied = tied;
  // A batch with an image table.  Evaluate mode: nothing per sample touches the maps (no dropout on X), so
  // i_embed and the attention pre-activation run once per IMAGE and the attention kernels read sample b's
  // tiles at row image_of[b].  Everywhere else (train mode: per-sample masks; a captured step: its backward
  // needs per-sample I) the table is gathered into per-sample maps first and the plain path runs on those.
  // (Nor under RAU_FEAT_GRAD_IMAGES: the per-image gradient differentiates per-sample I.  Same output bits.)
  const bool table_fwd = bs.held.n_images > 0 && ctx->fwd.I_shared && ctx->mode == RAU_MODE_EVAL && !ctx->capturing &&
                         !xgrad_per_image(ctx);
  const int nX = table_fwd ? bs.held.n_images : B;   // maps the image-side passes read
  const int32_t* img = table_fwd ? bs.image_of_d : nullptr;
  const float* feats = bs.feats;
  if (table_fwd && bs.held.bank && !bs.held.table_ok) {
    // a bank batch handed over in train mode carries its row index only: the table is gathered now
    const size_t map_bytes = (size_t)D * S * feat_elem_bytes(bs.held.feat_type);
    RUN("bank_gather", 0, 2.0 * nX * map_bytes,
        bank_gather(st, nX, map_bytes, ctx->bank, ctx->bank_cap, bs.bank_idx_d, bs.feats));
    bs.held.table_ok = true;
  }
  if (!table_fwd)
    if (int rc = batch_maps(ctx, &feats)) return rc;   // (on st, in front of evA: the bulk stream is ordered behind it)
  ctx->fwd.table = table_fwd;
  std::vector<int>& gsz = ctx->fwd.groups;
  gsz = ctx->groups;
  if (ctx->fwd.I_shared) { gsz.assign(H, 0); gsz[0] = H; }   // evaluate mode: one launch group
  // ---------------- bulk stream: everything about the feature map that does not depend on the recurrence (overlaps
  // the encoder and the hop loop below); in evaluate mode I is hop-invariant and computed once.  Hops are launched in
  // groups of `hop_group` so hop h's chain can start as soon as its group is done while this stream works on the rest.
  hipStream_t sb = ctx->st2;
  HIPC(hipEventRecord(ctx->evA, st));
  HIPC(hipStreamWaitEvent(sb, ctx->evA, 0));
  bool x16 = false;
  if (int rc = feature_maps(ctx, sb, m, feats, nX, &x16)) return rc;
  for (int h0 = 0; h0 < H; h0 += gsz[h0]) {
    const int nBI = ctx->fwd.I_shared ? nX : gsz[h0] * B;
    const size_t hb = ctx->fwd.I_shared ? 0 : (size_t)h0 * B;  // first (hop, sample) row
    const void* xin = x16 ? map_elems(ctx->xd16, true, hb * D * S) : m.x ? ctx->xd + hb * D * S : ctx->fwd.xw;
    if (int rc = image_forward(ctx, sb, nBI, xin, x16, ctx->I + hb * M * S,
                               ctx->fwd.I_shared ? ctx->P0 : ctx->T + hb * A * S))
      return rc;
    HIPC(hipEventRecord(ctx->evF[h0], sb));
  }
  // a question from the caller (rau_set_question_dev) stands where the encoder's output would: nothing of the encoder
  // is launched, the hop chain below is the same launch for launch
  if (!bs.held.question) {
    if (int rc = encoder_forward(ctx, m)) return rc;
    RUN("gather_q", 0, (double)B * Q * 8,
        gather_q(st, B, Rq, TL, bs.lens_d, ctx->c1, ctx->h1, ctx->c2, ctx->h2, ctx->q));
  }

  // ---------------- RAU hops, SS:467-520
  const size_t BM_ = (size_t)B * M, BR_ = (size_t)B * R;
  RUN("apply_mask", 0, (double)H * B * Q * 8,
      apply_mask(st, (size_t)H * B * Q, (size_t)B * Q, question_state(ctx), m.q, m.s_q, ctx->qd));
  bool q_split = false;
  {  // q_embed's question half (SS:233) for every hop clone; without dropout on q (evaluate mode) the
     // clones see the same rows: computed once
    ctx->fwd.yq_shared = (m.q == nullptr);
    // with dropout: hop 0's rows here, the other hops' rows on the weight-gradient stream (hop 1 waits)
    q_split = !ctx->fwd.yq_shared && side_split(ctx) && H > 1;
    const int qrows = (ctx->fwd.yq_shared || q_split) ? B : H * B;
    LinOpts o = lin_opts(ctx, ctx->ws_chain);
    o.bias = ctx->q_proj.b;
    o.bias2 = ctx->h_proj.b;
    RUN("q_proj_gemm", gflop(qrows, M, Q), 0,
        gemm_nt(st, qrows, M, Q, ctx->qd, Q, ctx->q_proj.W, Q, ctx->Yq, M, o));
  }
  if (q_split) {
    HIPC(hipEventRecord(ctx->evQ0, st));            // qd is complete
    HIPC(hipStreamWaitEvent(ctx->st3, ctx->evQ0, 0));
    LinOpts o = lin_opts(ctx, ctx->ws_side);
    o.bias = ctx->q_proj.b;
    o.bias2 = ctx->h_proj.b;
    RUNS(ctx->st3, "q_proj_gemm", gflop((H - 1) * B, M, Q), 0,
         gemm_nt(ctx->st3, (H - 1) * B, M, Q, ctx->qd + (size_t)B * Q, Q, ctx->q_proj.W, Q,
                 ctx->Yq + (size_t)B * M, M, o));
    HIPC(hipEventRecord(ctx->evQ, ctx->st3));
  }
  if (!bs.held.state) {   // (an attached initial state, rau_set_state_dev, lies in the two row blocks already)
    HIPC(hipMemsetAsync(ctx->cc, 0, BR_ * sizeof(float), st));  // att_c, att_h zeros SS:362-365
    HIPC(hipMemsetAsync(ctx->hh, 0, BR_ * sizeof(float), st));
  }
  const Truth truth = step_truth(ctx);
  // RAU_SEAM & 1: the heads are followed by the backward's two head products, unless that backward forms them itself
  const bool dpre = bs.held.have_labels && ctx->mode == RAU_MODE_TRAIN && (ctx->policy.seam & 1) && !bwd_forms_dpre;
  // rows the logits region of the head's workspace holds (hop_forward_head: a quarter of the side stream's slab)
  const int head_max = (int)std::max<size_t>(1, ctx->ws_side.floats / 4 / ((size_t)B * c.K));
  int gstart = 0;
  for (int h = 0; h < H; ++h) {
    if (gsz[h]) {
      HIPC(hipStreamWaitEvent(st, ctx->evF[h], 0));  // this group's I and P are ready
      gstart = h;
    }
    if (h == 1 && q_split) HIPC(hipStreamWaitEvent(st, ctx->evQ, 0));   // Yq rows of hops 1..
    if (int rc = hop_forward_chain(ctx, h, ctx->cc + (size_t)h * BR_, ctx->hh + (size_t)h * BR_,
                                   ctx->cc + (size_t)(h + 1) * BR_, ctx->hh + (size_t)(h + 1) * BR_,
                                   ctx->I + (ctx->fwd.I_shared ? 0 : (size_t)h * BM_ * S),
                                   ctx->fwd.I_shared ? ctx->P0 : ctx->T + (size_t)h * B * A * S, img,
                                   bs.held.regions ? bs.nreg_d : nullptr,
                                   bs.held.att_bias ? bs.zb_ext : nullptr))
      return rc;
    // classifier + criterion heads of the finished hops: nothing on the recurrence waits for
    // them, so they run on the weight-gradient stream (idle in the forward pass), batched over
    // the hops of a launch group
    const bool group_end = h + 1 == H || gsz[h + 1] != 0;
    if (group_end || h + 1 - gstart >= head_max) {
      HIPC(hipEventRecord(ctx->evH[h], st));
      HIPC(hipStreamWaitEvent(ctx->st3, ctx->evH[h], 0));
      if (int rc = forward_heads(ctx, gstart, h, head_max, truth, dpre)) return rc;
      gstart = h + 1;
    }
  }
  HIPC(hipEventRecord(ctx->evHd, ctx->st3));
  HIPC(hipStreamWaitEvent(st, ctx->evHd, 0));   // callers order against st only
  if (bs.held.have_labels)
    RUN("loss_reduce", 0, 0, loss_reduce(st, H, B, ctx->lossrow, ctx->losses_d));
  if (!ctx->capturing) merge_record(ctx);   // (rau_graph_step records behind its launch)
  ctx->fwd.done = true;
  ctx->fwd.dl = bs.held.have_labels;
  ctx->fwd.dpre = dpre;
  return RAU_OK;
}
int rau_forward(rau_ctx* ctx) { return forward_impl(ctx, false); }

// The caller's hop_w may be a temporary (and may be pinned memory, for which an async copy really
// is asynchronous): stage it in the ctx's own pinned buffer first.  Two slots, alternated, so the
// copy of step n is never overwritten by the host while step n+1's call prepares its own.
// The terms present travel behind hop_w in the same copy, each in its block of HopwLayout; an absent one in front
// of a present one goes as zeros.
static int upload_hop_weights(rau_ctx* ctx, const StepLoss& l) {
  const int H = ctx->cfg.H;
  const HopwLayout at(H);
  const int sl = (ctx->hopw_slot ^= 1);
  float* stage = ctx->hopw_h + (size_t)sl * at.size;
  // a host that runs two or more steps ahead of the device must not overwrite a staging slot whose
  // copy has not been read yet: wait for the copy issued from this slot two calls ago
  if (!ctx->hopw_ev[sl]) HIPC(hipEventCreateWithFlags(&ctx->hopw_ev[sl], hipEventDisableTiming));
  else HIPC(hipEventSynchronize(ctx->hopw_ev[sl]));
  const size_t count = l.merge_w ? at.size : l.att_w ? at.merge_w : l.select_w ? at.att_w : at.select_w;
  std::memset(stage, 0, count * sizeof(float));
  std::memcpy(stage, l.hop_w, (size_t)H * sizeof(float));
  if (l.select_w) std::memcpy(stage + at.select_w, l.select_w, (size_t)H * sizeof(float));
  if (l.att_w) std::memcpy(stage + at.att_w, l.att_w, (size_t)H * sizeof(float));
  if (l.merge_w) std::memcpy(stage + at.merge_w, l.merge_w, 2 * sizeof(float));
  HIPC(hipMemcpyAsync(ctx->hopw_d, stage, count * sizeof(float), hipMemcpyHostToDevice, ctx->st));
  if (!ctx->capturing) HIPC(hipEventRecord(ctx->hopw_ev[sl], ctx->st));
  return 0;
}

// =============================================================== backward
// The one place a backward with a select_w differs is marked `sel` below.  `att`: one launch, and HopGrad::da_out
// of every active hop.  `mrg`: one launch behind the hop scaling; like `sel` it is a per-row term, so dpre / dhn
// are formed here, and every hop is active (the uni row reads them all).
// `ext` (rau_backward_ext): caller-supplied gradients join dl behind its scaling (ext_dl, in scale_hops' place), s
// behind select_signal (ext_signal) and the attention addend behind att_sup_grad (ext_da); each of the three sites
// then runs with or without its built-in term.  Per-row terms again: dpre / dhn are formed here, every hop is active.
// The opening: from the loss terms to what the hop loop reads -- the final dl, the attention addend att_da and
// (unless the forward left them) dpre / dhn of the active hops.  `t`: the ground truth the forward's head read.
static int loss_gradients(rau_ctx* ctx, const StepLoss& loss, const Truth& t) {
  const bool sel = loss.select_w != nullptr, att = loss.att_w != nullptr, mrg = loss.merge_w != nullptr;
  const rau_out_grads& ext = loss.ext;
  const rau_config& c = ctx->cfg;
  const int B = c.B, S = ctx->Sp, SL = c.S, M = c.M, R = c.R, K = c.K, Kp = ctx->Kp, H = c.H, HA = loss.active;
  const HopwLayout at(H);
  const BatchSlot& bs = cur_batch(ctx);
  hipStream_t st = ctx->st;
  // dpred:mul(w[h])  SS:569 / MS:568-570 / Full:587-589
  if (!ctx->capturing)   // (rau_graph_step uploads the weights before it launches the graph)
    if (int rc = upload_hop_weights(ctx, loss)) return rc;
  if (ext.d_logits || (loss.external() && !ctx->fwd.dl))
    // one pass in scale_hops' place: dl * hop_w + d_logits; without a criterion gradient dl = d_logits (or +0)
    RUN("ext_dl", (double)H * B * K * (ctx->fwd.dl ? 2 : 0), (double)H * B * K * (ctx->fwd.dl ? 12 : 8),
        ext_dl(st, H, (size_t)B, K, Kp, ctx->fwd.dl ? ctx->hopw_d : nullptr, ext.d_logits, ctx->dl));
  else if (ctx->fwd.dpre && !loss.forms_dpre())   // the forward formed dpre / dhn from the unscaled dl: scale all three
    RUN("scale_hops", 0, (double)H * B * (K + M + R) * 8,
        scale_hops3(st, H, ctx->hopw_d, (size_t)B * Kp, ctx->dl, (size_t)B * M, ctx->dpre, (size_t)B * R, ctx->dhn));
  else
    RUN("scale_hops", 0, (double)H * B * K * 8, scale_hops(st, H, (size_t)B * Kp, ctx->hopw_d, ctx->dl));
  // mrg: w_uni dCE(uni row) + w_sel dCE(select row) join the scaled dl of every hop, in front of all its consumers
  // (head_dgrad and sel_add below, the classifier's weight gradient in mult_wgrads)
  if (mrg)
    RUN("merge_grad", 0, (double)H * B * K * 16,
        merge_grad(st, H, B, K, ctx->logits, ctx->dopred, t, ctx->hopw_d + at.merge_w, 0.f, 0.f, ctx->dl, Kp));
  // ---------------- RAU BPTT, SS:561-578
  // Off the recurrence: dpre = (dl Wc) (.) mask and dhn = dpre Wo for all active hops at once.
  // sel: the gradient through do_pred, s (x) wd, joins dl Wc in front of the mask (HopGrad::dmf_add's position).
  // A per-row term cannot be folded into what the forward formed (one scale per hop), so both products are
  // formed here from the scaled dl -- which is also the order the bf16 emulation rounds in.
  if (sel)
    RUN("select_signal", 0, (double)HA * B * M * 4,
        select_signal(st, HA * B, B, K, M, ctx->dopred, ctx->argmax_d, t, ctx->hopw_d + at.select_w, ctx->do_pred.W,
                      ctx->sel_s, ctx->sel_add));
  if (ext.d_dopred)   // s (+)= (d_dopred x)(1 - x) through the sigmoid, and the addend formed from the final s
    RUN("ext_signal", 0, (double)HA * B * M * 4,
        ext_signal(st, HA * B, M, ctx->dopred, ext.d_dopred, ctx->do_pred.W, sel, ctx->sel_s, ctx->sel_add));
  // att: the gradient at the attprob output of all active hops, -(att_w[h] t / (a + eps)) / B, read by the attention
  // backward of each hop (HopGrad::da_out).  The targets may have come after the forward: it does not read them.
  if (att)
    RUN("att_sup_grad", 0, (double)HA * B * S * 12,
        att_sup_grad(st, HA, B, SL, ctx->a, S, bs.att_t_d, S, bs.held.regions ? bs.nreg_d : nullptr,
                     ctx->hopw_d + at.att_w, 0.f, ctx->att_da, S, t.sw));
  if (ext.d_attprob)   // the dense [H,n,S] gradient (added) into the pitched addend, zeros behind the counts
    RUN("ext_da", 0, (double)HA * B * S * (att ? 12 : 8),
        ext_da(st, HA, B, SL, ext.d_attprob, bs.held.regions ? bs.nreg_d : nullptr, att, ctx->att_da, S));
  if (HA > 0 && (!ctx->fwd.dpre || loss.forms_dpre()))
    return head_dgrad(ctx, ctx->ws_chain, 0, HA, (sel || ext.d_dopred) ? ctx->sel_add : nullptr);
  return RAU_OK;
}

// The feature-map gradient of `nh` hops from hop h0 on (rau_set_feat_grad), on the bulk stream behind the conv
// gradients that formed their dZ: xg_dX (=, for the backward's first launch, `first`, else +=) sum_h keep_h s_x Wi^T dZ_h.
// dz: hop h0's [B][M][Sp] block, nh of them; is_dI: it holds the gradient at i_embed's OUTPUT (the dgrad without
// the fused tanh derivative), I the matching activations (I_stride floats from hop to hop, 0 = shared).
// mask_hop: the first hop's slice of the mask site (tied: 0), mask_step hops per hop (tied, no mask: 0).
// RAU_FEAT_GRAD_IMAGES on an image table (xgrad_per_image): the same products, added per image into xg_dX as
// [slots][D][Sp] in the order of the slot's sample lists; launched over the capacity's slots, whatever N is.
static int feat_grad_hops(rau_ctx* ctx, hipStream_t sb, int nh, const void* dz, bool dz_is_b16, bool is_dI,
                          const float* I, size_t I_stride, int mask_hop, int mask_step, bool& first) {
  const rau_config& c = ctx->cfg;
  const int B = c.B, D = c.D, S = ctx->Sp, SL = c.S, M = c.M;
  const Masks m = masks_of(ctx);
  XMask xm{};
  xm.kind = !m.x ? 0 : ctx->fwd.xgen ? 2 : 1;
  xm.bits = m.x;
  xm.hop_stride = (size_t)B * D * SL;
  xm.seed = ctx->seed; xm.site = RAU_MASK_X; xm.step = ctx->step; xm.key = ctx->dkey;
  xm.thr = (uint32_t)lroundf(ctx->mp[RAU_MASK_X] * 256.0f);
  xm.scale = m.x ? m.s_x : 1.f;
  const double fl = gflop(D, (double)B * S, M), by = ((double)B * M * S + (double)B * D * S) * 4;
  const bool per_image = xgrad_per_image(ctx);   // (never fused: that kernel owns one sample's tile)
  const BatchSlot& bs = cur_batch(ctx);
  if (!per_image && !dz_is_b16 && !is_dI && !ctx->bf16 && xgrad_fused_ok(ctx->policy.xgrad_fused, D, M, S) && S == SL) {
    xm.e0 = (size_t)mask_hop * xm.hop_stride;
    if (!mask_step) xm.hop_stride = 0;
    RUNS(sb, "conv_embed_dgrad", nh * fl, (double)nh * B * M * S * 4 + (double)B * D * S * (first ? 4 : 8),
         xgrad_fused(sb, nh, B, D, M, S, (const float*)dz, ctx->i_embed.W, ctx->xg_dX, xm, first ? 1 : 0));
    first = false;
    return RAU_OK;
  }
  for (int k = 0; k < nh; ++k) {
    const void* dzk = map_elems(const_cast<void*>(dz), dz_is_b16, (size_t)k * B * M * S);
    if (is_dI) {
      RUNS(sb, "mul_dtanh", 0, (double)B * M * S * 12,
           mul_dtanh(sb, (size_t)B * M * S, (const float*)dzk, I + (size_t)k * I_stride, ctx->xg_dz));
      dzk = ctx->xg_dz;
    }
    RUNS(sb, "conv_embed_dgrad", fl, by,
         conv_embed_dgrad_mode(sb, conv_mode(ctx), B, D, S, M, dzk, dz_is_b16 ? 1 : 0, ctx->i_embed.W, ctx->xg_tmp));
    xm.e0 = (size_t)(mask_hop + k * mask_step) * xm.hop_stride;
    if (per_image)
      RUNS(sb, "xgrad_accum_img", 2.0 * B * D * S,
           ((double)B * 4 + (double)bs.held.n_images * (first ? 4 : 8)) * D * S,
           xgrad_accum_img(sb, ctx->cap, D, SL, S, ctx->xg_tmp, ctx->xg_dX, bs.img_start_d, bs.img_samples_d, xm,
                           first ? 1 : 0));
    else
      RUNS(sb, "xgrad_accum", 2.0 * B * D * S, (double)B * D * S * (first ? 8 : 12),
           xgrad_accum(sb, (size_t)B * D, SL, S, ctx->xg_tmp, ctx->xg_dX, xm, first ? 1 : 0));
    first = false;
  }
  return RAU_OK;
}

// The 1x1-conv gradients of the launch group that starts with hop h, on the bulk stream (dZ feeds the weight
// gradients; the feature-map gradient is dead in the reference, SS:579, and formed only under rau_set_feat_grad:
// feat_grad_hops above, which owns dX_first); HA = the active hops; ds16: the hops left their dS as bf16 (HopGrad::ds16).
static int group_conv_grads(rau_ctx* ctx, int h, int group, int HA, bool ds16, bool& dX_first) {
  const rau_config& c = ctx->cfg;
  const int B = c.B, D = c.D, S = ctx->Sp, M = c.M, A = c.A;
  hipStream_t sb = ctx->st2;
  ConvGrads g{};
  if (!ctx->fwd.I_shared) {
    const size_t hb = (size_t)h * B;
    g.n = (std::min(h + group, HA) - h) * B;   // active hops of this group
    g.dzf = conv_dz_fused_ok(conv_mode(ctx), S, M);
    g.ds_is_b16 = ds16;
    g.dS = g.ds_is_b16 ? map_elems(ctx->dS16, true, hb * A * S) : ctx->T + hb * A * S;
    g.dj = ctx->dj + hb * M; g.a = ctx->a + hb * S; g.I = ctx->I + hb * M * S;
    g.x_is_b16 = g.dz_is_b16 = ctx->xd16 && g.dzf;
    g.X = g.x_is_b16 ? map_elems(ctx->xd16, true, hb * D * S) : ctx->xd + hb * D * S;
    g.dZ = map_elems(ctx->dZ, g.dz_is_b16, hb * M * S);
    g.dbi_part = ctx->dbi_part + hb * M;
    if (int rc = conv_grads(ctx, sb, g)) return rc;
    if (g.dzf && h == 0)   // last group: i_embed bias gradient = column sums of the per-sample rows
      RUNS(sb, "colsum", 0, (double)HA * B * M * 4,
           colsum_acc(sb, HA * B, M, ctx->dbi_part, M, ctx->i_embed.db, ctx->ws_bulk.coltmp));
    if (ctx->feat_grad)
      return feat_grad_hops(ctx, sb, g.n / B, g.dZ, g.dz_is_b16, !g.dzf, g.I, (size_t)B * M * S, h, 1, dX_first);
    return RAU_OK;
  }
  g.n = B; g.I = ctx->I;
  if (ctx->fwd.tied) {
    // Tied feature-map dropout (train mode, I and X' shared): the conv gradients are linear in what each hop
    // hands back, so the hops are summed first (tied_bwd.hip) and every conv gradient runs once, at n = B.
    // The sum of dS goes to a buffer of its own: T keeps every hop's dS, as on the per-hop paths.
    RUNS(sb, "hop_sum", 0, (double)(HA + 1) * B * A * S * 4, hop_sum(sb, HA, B, A, c.S, S, ctx->T, ctx->dS_sum));
    g.dS = ctx->dS_sum; g.dj = ctx->dj; g.a = ctx->a; g.X = ctx->fwd.x_shared; g.dZ = ctx->dZ; g.tied_hops = HA;
    if (int rc = conv_grads(ctx, sb, g)) return rc;
    // one mask: keep * s_x * Wi^T (sum_h dZ_h), and dZ holds that sum (as dI: the tanh derivative is hop-invariant)
    if (ctx->feat_grad) return feat_grad_hops(ctx, sb, 1, ctx->dZ, false, true, ctx->I, 0, 0, 0, dX_first);
    return RAU_OK;
  }
  for (int hh2 = 0; hh2 < HA; ++hh2) {  // evaluate mode: I (and X) shared by all hops
    const size_t hb = (size_t)hh2 * B;
    g.dS = ctx->T + hb * A * S; g.dj = ctx->dj + hb * M; g.a = ctx->a + hb * S;
    g.X = ctx->fwd.xw; g.dZ = ctx->dZ + hb * M * S;
    if (int rc = conv_grads(ctx, sb, g)) return rc;
  }
  if (ctx->feat_grad && HA > 0)   // no mask, scale 1: the hops in ascending order
    return feat_grad_hops(ctx, sb, HA, ctx->dZ, false, true, ctx->I, 0, 0, 0, dX_first);
  return RAU_OK;
}

// ---------------- mult-group weight gradients, one GEMM per weight over all active hops, on the stream and with
// the scratch of one record (wg_bulk & 1: the bulk stream's).  sig: the selection head's weight gradient exists.
static int mult_wgrads(rau_ctx* ctx, int HA, bool sig, int wg_bulk) {
  const rau_config& c = ctx->cfg;
  const int B = c.B, S = ctx->Sp, SL = c.S, M = c.M, A = c.A;
  const StreamWs& ws = (wg_bulk & 1) ? ctx->ws_bulk : ctx->ws_side;
  hipStream_t sw = ws.owner;
  HIPC(hipStreamWaitEvent(sw, ctx->evW, 0));
  const int rows = HA * B;                 // active hops only
  if (rows == 0) {
    HIPC(hipEventRecord(ctx->evM3, sw));
    return 0;
  }
  TnProblem pr[13];   // dW += dY^T X and db += column sums of dY for the nine Linears: one grouped launch
  const int np = mult_wgrad_problems(ctx, pr);
  double fl = 0;
  for (int i = 0; i < np; ++i) fl += gflop(pr[i].M, pr[i].N, rows);
  RUNS(sw, "wgrad_gemm", fl, 0, gemm_tn_group_acc(sw, pr, np, rows, ws.slab, ws.floats, lin_mode(ctx).bf16));
  if (sig)   // the head's own weights: dwd += sum s mf, dbd += sum s (f32 dot products in every dtype)
    RUNS(sw, "select_wgrad", 2.0 * rows * (M + 1), (double)rows * M * 4,
         select_wgrad(sw, rows, M, ctx->sel_s, ctx->mf, ctx->do_pred.dW, ctx->do_pred.db));
  // att_score: dws = sum dz T ; dbs = sum dz.  att_i bias: sum dS.  i_embed bias: sum dZ.
  RUNS(sw, "colsum", 0, (double)rows * A * 4, colsum_acc(sw, rows, A, ctx->dwsp, A, ctx->att_score.dW, ws.coltmp));
  HIPC(hipMemsetAsync(ctx->tmpS, 0, S * sizeof(float), sw));
  RUNS(sw, "colsum", 0, (double)rows * S * 4, colsum_acc(sw, rows, SL, ctx->dz, S, ctx->tmpS, ws.coltmp));
  RUNS(sw, "colsum", 0, S * 4.0, colsum_acc(sw, SL, 1, ctx->tmpS, 1, ctx->att_score.db, ws.coltmp));
  RUNS(sw, "colsum", 0, (double)rows * A * 4, colsum_acc(sw, rows, A, ctx->du, A, ctx->att_i.db, ws.coltmp));
  HIPC(hipEventRecord(ctx->evM3, sw));   // with evD: the mult group's gradients are final
  return 0;
}

// Encoder weight gradients of all TL tokens, also on the weight-gradient stream (wg_bulk & 2: the bulk stream):
// one launch behind the BPTT.  (Two time chunks -- the gradients of tokens t > uc are final once wavefront step
// uc is done -- were tried: running the first chunk under the second half of the BPTT slows that chain by more
// than the shorter tail saves, measured 11.05 vs 10.6 ms.)
static int enc_wgrads(rau_ctx* ctx, int TL, int wg_bulk) {
  const StreamWs& ws = (wg_bulk & 2) ? ctx->ws_bulk : ctx->ws_side;
  hipStream_t sw = ws.owner;
  HIPC(hipEventRecord(ctx->evE, ctx->st));
  HIPC(hipStreamWaitEvent(sw, ctx->evE, 0));
  const int nr = TL * ctx->cfg.B;
  TnProblem pr[13];
  const int np = enc_wgrad_problems(ctx, 0, pr);
  double fl = 0;
  for (int i = 0; i < np; ++i) fl += gflop(pr[i].M, pr[i].N, nr);
  RUNS(sw, "wgrad_gemm", fl, 0, gemm_tn_group_acc(sw, pr, np, nr, ws.slab, ws.floats, lin_mode(ctx).bf16));
  return 0;
}

// ---------------- encoder BPTT, SS:581-596 -- the same two-layer wavefront, reversed:
// step u handles layer-2 cell u and layer-1 cell u+1; their incoming dh are the
// K-split partials of the previous step's dG (dG2 W_h2h2, dG2 W_i2h2 through the
// inter-layer dropout, dG1 W_h2h1), one batched GEMM, summed inside the cell kernel.
// Then the gradient at the word embeddings and the encoder's weight gradients.
static int encoder_backward(rau_ctx* ctx, const Masks& m, int wg_bulk) {
  const BatchSlot& bs = cur_batch(ctx);
  const rau_config& c = ctx->cfg;
  const int B = c.B, E = c.E, Rq = c.Rq, Q = ctx->Q, TL = bs.held.max_len;
  const size_t BRq = (size_t)B * Rq;
  hipStream_t st = ctx->st;
  if (TL <= 0) return RAU_OK;
  const int rows = TL * B;
  const size_t G4 = (size_t)B * 4 * Rq;
  for (int u = TL; u >= 0; --u) {
    const float* Ap[3];
    const float* Wp[3];
    int nb = 0, iq2 = -1, iqx = -1, iq1 = -1;
    if (u >= 1 && u + 1 <= TL) { Ap[nb] = ctx->dG2 + (size_t)u * G4; Wp[nb] = ctx->h2h[1].W; iq2 = nb++; }
    if (u + 1 <= TL) { Ap[nb] = ctx->dG2 + (size_t)u * G4; Wp[nb] = ctx->i2h[1].W; iqx = nb++; }
    if (u + 2 <= TL) { Ap[nb] = ctx->dG1 + (size_t)(u + 1) * G4; Wp[nb] = ctx->h2h[0].W; iq1 = nb++; }
    int nsp = 0;
    if (nb > 0)
      RUN("enc_h2h_dgrad", gflop(B, Rq, 4 * Rq) * nb, 0,
          gemm_nn_batched_deferred(st, lin_mode(ctx), nb, B, Rq, 4 * Rq, Ap, 4 * Rq, Wp, Rq, ctx->ws_chain.slab,
                                   ctx->ws_chain.floats, &nsp));
    LstmBwdCells cells{};
    cells.lens = bs.lens_d;
    cells.dq_rs = Q;
    if (u >= 1) {  // layer-2 cell t = u
      LstmBwdCell& C2 = cells.c[cells.n++];
      C2.gates = ctx->G2 + (size_t)(u - 1) * G4;
      C2.c_prev = ctx->c2 + (size_t)(u - 1) * BRq; C2.cp_rs = Rq;
      C2.tanhc = ctx->tc2 + (size_t)(u - 1) * BRq;
      C2.slabA = iq2 >= 0 ? ctx->ws_chain.slab + (size_t)iq2 * nsp * BRq : nullptr;
      C2.nA = iq2 >= 0 ? nsp : 0;
      C2.slabB = nullptr; C2.nBp = 0; C2.maskB = nullptr; C2.maskB_e0 = 0; C2.mscaleB = 1.f;
      C2.dc_next = u < TL ? ctx->edc[1][(u + 1) & 1] : nullptr;
      C2.dsum = ctx->dG2 + (size_t)(u - 1) * G4;
      C2.dc_prev = ctx->edc[1][u & 1];
      C2.t = u; C2.dq_c = ctx->dq + 2 * Rq; C2.dq_h = ctx->dq + 3 * Rq;
    }
    if (u + 1 <= TL) {  // layer-1 cell t = u + 1
      const int t = u + 1;
      LstmBwdCell& C1 = cells.c[cells.n++];
      C1.gates = ctx->G1 + (size_t)u * G4;
      C1.c_prev = ctx->c1 + (size_t)u * BRq; C1.cp_rs = Rq;
      C1.tanhc = ctx->tc1 + (size_t)u * BRq;
      C1.slabA = iq1 >= 0 ? ctx->ws_chain.slab + (size_t)iq1 * nsp * BRq : nullptr;
      C1.nA = iq1 >= 0 ? nsp : 0;
      C1.slabB = ctx->ws_chain.slab + (size_t)iqx * nsp * BRq;   // dG2[t] W_i2h2, then the dropout mask
      C1.nBp = nsp;
      C1.maskB = m.rnn; C1.maskB_e0 = (size_t)u * BRq; C1.mscaleB = m.s_rnn;
      C1.dc_next = t < TL ? ctx->edc[0][(t + 1) & 1] : nullptr;
      C1.dsum = ctx->dG1 + (size_t)u * G4;
      C1.dc_prev = ctx->edc[0][t & 1];
      C1.t = t; C1.dq_c = ctx->dq; C1.dq_h = ctx->dq + Rq;
    }
    RUN("lstm_bwd", 0, BRq * 4.0 * 12 * cells.n, lstm_bwd_multi(st, GATES_DEEP, B, Rq, cells));
  }
  {  // gradient w.r.t. the word embeddings' tanh output, all tokens at once
    const LinOpts o = lin_opts(ctx, ctx->ws_chain);
    RUN("enc_i2h_dgrad", gflop(rows, E, 4 * Rq), 0,
        gemm_nn(st, rows, E, 4 * Rq, ctx->dG1, 4 * Rq, ctx->i2h[0].W, E, ctx->dwe, E, o));
  }
  RUN("embed_bwd", 0, (double)rows * E * 12,
      embed_bwd(st, ctx->capturing ? c.T * B : bs.held.nuniq, E, bs.utok, bs.ustart, bs.upos, ctx->dwe, ctx->we, m.we,
                m.s_we, ctx->grp[RAU_GROUP_EMBED].g));
  return enc_wgrads(ctx, TL, wg_bulk);
}

// A step-level backward on the resident batch has been enqueued (graph: as a graph launch): what the getters may read
static void record_backward(rau_ctx* ctx, bool graph) {
  const BatchDesc& d = cur_batch(ctx).held;
  ctx->bwd.done = true;
  ctx->bwd.graph = graph;
  ctx->bwd.dq = d.question;
  ctx->bwd.dstate = d.state;
  ctx->bwd.dbias = d.att_bias;
  ctx->bwd.dX = ctx->feat_grad != RAU_FEAT_GRAD_OFF;
  ctx->bwd.dX_rows = xgrad_per_image(ctx) ? d.n_images : ctx->cfg.B;
}

static int backward_impl(rau_ctx* ctx, const StepLoss& loss) {
  const bool sel = loss.select_w != nullptr, att = loss.att_w != nullptr, mrg = loss.merge_w != nullptr;
  const rau_out_grads& ext = loss.ext;
  const bool sig = sel || ext.d_dopred;   // the head_dgrad addend and the selection head's weight gradient exist
  const bool has_da = att || ext.d_attprob;   // every hop's attention backward is handed its da_out
  const int HA = loss.active;
  if (!ctx->fwd.done) return fail(RAU_ERR_STATE, "rau_backward: call rau_forward first");
  if (ctx->fwd.table)
    return fail(RAU_ERR_STATE, "rau_backward: the evaluate-mode forward of a batch with an image table computed "
                "i_embed once per image, so there is no per-sample I to differentiate; take evaluate-mode "
                "gradients on a plain batch (rau_set_batch)");
  const BatchSlot& bs = cur_batch(ctx);
  if (ctx->feat_grad && bs.held.n_images > 0 && !xgrad_per_image(ctx))
    return fail(RAU_ERR_STATE, "rau_backward: the feature-map gradient (rau_set_feat_grad) of a batch with an image "
                "table or bank rows is a sum over the questions of an image, which is not formed; expand the maps "
                "per sample (rau_set_batch_dev) or turn the switch off");
  // the feature-map keep bits that forward drew in its dropout pass exist nowhere: the backward regenerates them
  // from the key, which must still be that forward's (a captured step holds both passes: the key cannot move)
  if (ctx->feat_grad && !ctx->capturing && ctx->fwd.xgen && masks_of(ctx).x &&
      (ctx->seed != ctx->fwd.seed || ctx->step != ctx->fwd.step))
    return fail(RAU_ERR_STATE, "rau_backward: rau_set_dropout_seed was called between the forward and this backward; "
                "with the feature-map gradient on (rau_set_feat_grad) the backward regenerates the forward's "
                "feature-map dropout bits from the key: run the forward again");
  // an external-only backward reads no label: hop_w zeros, no select_w, no merge_w (att_w reads the targets alone)
  const bool builtin = !loss.external() || loss.hop_any || sel || mrg;
  if (builtin && !bs.held.have_labels) return fail(RAU_ERR_STATE, "rau_backward: batch has no labels");
  if (builtin && loss.external() && !ctx->fwd.dl)
    return fail(RAU_ERR_STATE, "rau_backward_ext: the forward ran on a batch without labels, so there is no "
                "criterion gradient for a non-zero hop_w, select_w or merge_w");
  // the head's target is read from that forward's labels or answer set: they must still be there (a captured
  // step reads the resident batch, which rau_graph_step_select has checked)
  if ((sel || mrg) && !ctx->capturing)
    if (int rc = merge_state(ctx, sel ? "rau_backward_select" : "rau_backward_merged", true)) return rc;
  const Truth t = ctx->capturing ? step_truth(ctx) : ctx->mg.truth;
  const rau_config& c = ctx->cfg;
  const int B = c.B, S = ctx->Sp, M = c.M, R = c.R, Q = ctx->Q;
  // Backward launch groups of the bulk stream.  Forward groups want to be large (the flattened-
  // column kernels lose a ragged last round per launch); the backward kernels do not (per-sample
  // dgrad tiles and the split-K weight gradients fill whole rounds at any hop count), and a
  // group's gradients can only start once its LAST hop's chain is done, so the backward partition
  // is its own: RAU_BWD_GROUPS="1,1,2,2,2" (sizes in HOP order, must sum to H), default = the
  // forward partition.  Evaluate mode (I shared): one group.
  const std::vector<int>& gsz = (!ctx->fwd.I_shared && !ctx->bgroups.empty()) ? ctx->bgroups : ctx->fwd.groups;
  hipStream_t st = ctx->st;
  const Masks m = masks_of(ctx);
  const size_t BM_ = (size_t)B * M, BS_ = (size_t)B * S, BR_ = (size_t)B * R;
  drop_forward(ctx);      // dl is scaled in place below: one backward per forward
  bool dX_first = true;   // (feat_grad) the first launch that writes xg_dX stores, the others add
  if (int rc = loss_gradients(ctx, loss, t)) return rc;
  // grad_att_c / grad_att_h zeros, SS:561-562; or the caller's gradients at the states (rau_backward_state: every
  // hop is active then, so the loop's first hop is the last one)
  const float* dc_next = loss.sg.d_c_last;
  const bool state = bs.held.state;   // an attached initial state (rau_set_state_dev): its gradient is a result
  float* dh_part = nullptr;        // gradient at next_h: K-split partials left by the previous hop
  int dh_part_ns = 0;
  // bf16 mode, train-mode step on 14x14 maps: dS goes out as bf16 (its consumers below read that)
  const bool ds16 = ctx->dS16 && !ctx->fwd.I_shared && !ctx->att_split && conv_dz_fused_ok(conv_mode(ctx), S, M);
  bool dq_side = false;
  int dq_rows_left = HA;           // hops [0, dq_rows_left) whose dq term this stream still owes
  for (int h = HA - 1; h >= 0; --h) {
    float* dc_out = ctx->dcn[h & 1];
    {
      HopGrad g{};
      g.dl = ctx->dl + (size_t)h * B * ctx->Kp;
      g.dc_next = dc_next;
      g.dc_out = dc_out;
      g.dpre_ready = 1;
      g.dhn_all = ctx->dhn;
      g.dh_part = dh_part;
      g.dh_part_ns = dh_part_ns;
      g.dh_part_out = &dh_part;
      g.dh_part_ns_out = &dh_part_ns;
      // h is the first hop of its launch group: its conv gradients may start behind att_bwd, three launches
      // before the hop's backward is over (it matters for the first group: the forward / backward seam)
      g.ev_conv_ready = (gsz[h] && (ctx->policy.seam & 2)) ? ctx->evK[h] : nullptr;
      g.dh_next = loss.sg.d_h ? loss.sg.d_h + (size_t)h * BR_ : nullptr;
      // hop 0's prev_h is the constant initial state: nothing reads its gradient -- but for an attached one's caller
      g.dh_prev_dead = h == 0 && !state;
      g.da_out = has_da ? ctx->att_da + (size_t)h * BS_ : nullptr;
      g.ds16 = ds16;
      if (int rc = hop_backward(ctx, h, ctx->cc + (size_t)h * BR_,
                                ctx->I + (ctx->fwd.I_shared ? 0 : (size_t)h * BM_ * S), g))
        return rc;
    }
    dc_next = dc_out;
    if (h == 0 && state)   // d_h0 = hop 0's dh_prev partials summed, d_c0 = its dc_prev: out of the workspace at once
      RUN("state_grad_finish", (double)dh_part_ns * BR_, (double)(dh_part_ns + 3) * BR_ * 4,
          state_grad_finish(st, BR_, dh_part, dh_part_ns, dc_out, ctx->sgrad, ctx->sgrad + (size_t)ctx->cap * R));
    // dq's per-hop terms dq~_h Wq (ConcatTable backward, SS:579) do not feed the recurrence: the
    // rows of a finished hop group go to the weight-gradient stream (idle until the hop loop
    // ends); only the last group's stay on this stream, in front of dq_reduce below
    if (gsz[h] && h > 0 && side_split(ctx)) {
      const int nh = std::min(h + gsz[h], HA) - h;
      HIPC(hipEventRecord(ctx->evK[h], st));
      HIPC(hipStreamWaitEvent(ctx->st3, ctx->evK[h], 0));
      const LinOpts o = lin_opts(ctx, ctx->ws_side);
      RUNS(ctx->st3, "q_proj_dgrad", gflop(nh * B, Q, M), 0,
           gemm_nn(ctx->st3, nh * B, Q, M, ctx->dqt + (size_t)h * BM_, M, ctx->q_proj.W, Q,
                   ctx->dQD + (size_t)h * B * Q, Q, o));
      HIPC(hipEventRecord(ctx->evDq, ctx->st3));
      dq_side = true;
      dq_rows_left = h;       // hops [0, h) are still to do
    }
    // ---------------- bulk stream: the 1x1-conv gradients are off the recurrence's
    // critical path (dZ only feeds weight gradients; the feature-map gradient is dead,
    // SS:579, never formed).  As soon as a hop group's chain is done its conv gradients
    // start on the bulk stream, overlapping the remaining hops and the encoder BPTT:
    // dZ = (Wp^T dS + dj (x) a)(1 - I^2); dWp += dS I^T; dWi += dZ X'^T.
    if (gsz[h]) {   // h is the first hop of its group: the whole group's attention backward is done
      if (!(ctx->policy.seam & 2)) HIPC(hipEventRecord(ctx->evK[h], st));
      HIPC(hipStreamWaitEvent(ctx->st2, ctx->evK[h], 0));   // recorded inside hop_backward (ev_conv_ready)
      if (int rc = group_conv_grads(ctx, h, gsz[h], HA, ds16, dX_first)) return rc;
    }
  }
  {  // dq = sum_h (dq~_h Wq) (.) mask_h     (ConcatTable backward, SS:579)
    const LinOpts o = lin_opts(ctx, ctx->ws_chain);
    if (dq_rows_left > 0)
      RUN("q_proj_dgrad", gflop(dq_rows_left * B, Q, M), 0,
          gemm_nn(st, dq_rows_left * B, Q, M, ctx->dqt, M, ctx->q_proj.W, Q, ctx->dQD, Q, o));
    if (dq_side) HIPC(hipStreamWaitEvent(st, ctx->evDq, 0));
    RUN("dq_reduce", 0, (double)HA * B * Q * 4,
        dq_reduce(st, HA, (size_t)B * Q, ctx->dQD, m.q, m.s_q, ctx->dq));
  }
  if (state && HA == 0) HIPC(hipMemsetAsync(ctx->sgrad, 0, (size_t)2 * ctx->cap * R * sizeof(float), st));
  // an attached attention bias (rau_set_att_bias_dev): its gradient is the active hops' dz summed in ascending order,
  // all of them resident behind the hop loop (mult_wgrads below reads the same rows); exact zeros without an active hop
  if (bs.held.att_bias)
    RUN("att_bias_grad", (double)HA * B * S, (double)(HA + 1) * B * S * 4,
        att_bias_grad(st, HA, B, c.S, S, ctx->dz, (size_t)B * S, ctx->zbgrad));
  // no active hop: the gradient is zero (n rows: all of a table's N <= n too, whichever N a replay meets)
  if (ctx->feat_grad && dX_first)
    HIPC(hipMemsetAsync(ctx->xg_dX, 0, (size_t)B * c.D * S * sizeof(float), ctx->st2));
  // rau_set_feat_norm: xg_dX holds the gradient at the normalised maps; back through the normalisation, in place.
  // Per image (xgrad_per_image) every slot of the capacity, like the accumulate pass: slot i reads the xn of its
  // list's first sample (all of them are that image's map), a slot without samples keeps its zeros.
  if (ctx->feat_grad && ctx->xnorm) {
    const bool per_image = xgrad_per_image(ctx);
    const int rows = per_image ? ctx->cap : B;
    RUNS(ctx->st2, "l2norm_backward", 5.0 * rows * c.D * S, (double)rows * c.D * S * 12,
         l2norm_backward(ctx->st2, rows, c.D, c.S, S, ctx->xn, ctx->nrm, ctx->xnorm_eps, ctx->xg_dX,
                         per_image ? bs.img_start_d : nullptr, per_image ? bs.img_samples_d : nullptr));
  }
  // bulk stream tail: the join event (the i_embed bias gradient comes out of conv_embed_wgrad:
  // row sums of its staged dZ operand)
  HIPC(hipEventRecord(ctx->evD, ctx->st2));
  // ---------------- mult-group weight gradients, one GEMM per weight over all hops.
  // Throughput work nothing else waits for: third stream, so the encoder BPTT (the
  // long latency-bound chain) starts right after dq instead of behind ~40 launches.
  HIPC(hipEventRecord(ctx->evW, st));
  // Where the grouped Linear weight-gradient GEMMs run.  Two MFMA-bound kernels side by side share one
  // matrix pipe: the round-3 timeline shows the mult group's GEMM (943 us beside the bulk stream, ~500
  // alone) and the conv weight gradient it overlaps (827 us instead of ~450) each at about half their
  // stand-alone rate, i.e. nothing is gained by overlapping them, and the recurrence's kernels then
  // compete with two heavy kernels instead of one.  Where the bulk stream is the longer path (f32 step,
  // more than 64 samples) the mult group's GEMM therefore goes to the END of the bulk stream, behind the
  // last conv gradient (round 4: 9.43 -> 9.38 ms with dgrad_dma.hip; conv_att_dgrad 0.47 -> 0.54 and
  // conv_att_wgrad 0.57 -> 0.60 of peak in the step).  The encoder group's GEMM (after the BPTT) measured
  // the same on either stream and stays on the third.  RAU_WG_BULK=<mask> overrides (A/B, DESIGN.md section
  // 8): 1 = mult group on the bulk stream, 2 = encoder group too.  Not with the side-stream split (the
  // third stream's split-K workspace would be shared).  Each group takes the stream AND the scratch of one record.
  const int wg_env = ctx->policy.wg_bulk;
  const int wg_bulk = side_split(ctx) ? 0 : wg_env >= 0 ? wg_env : (chain_bound(ctx) ? 0 : 1);
  if (int rc = mult_wgrads(ctx, HA, sig, wg_bulk)) return rc;
  // an attached question (rau_set_question_dev): dq above is the result, handed to the caller; no BPTT, no embedding
  // gradient, no encoder weight-gradient GEMM -- the EMBED and RNN gradient buffers are not touched.  The joins
  // below stand as they are: evW3 closes the third stream behind whatever it still runs (the mult group's block
  // unless wg_bulk & 1), evD the bulk stream, and evEnd then covers all three groups.
  if (!bs.held.question)
    if (int rc = encoder_backward(ctx, m, wg_bulk)) return rc;
  HIPC(hipEventRecord(ctx->evW3, ctx->st3));
  HIPC(hipStreamWaitEvent(st, ctx->evW3, 0));
  if (wg_bulk) HIPC(hipEventRecord(ctx->evD, ctx->st2));   // the bulk stream got weight-gradient work behind its convs
  HIPC(hipStreamWaitEvent(st, ctx->evD, 0));  // join: every gradient is ordered on st
  HIPC(hipEventRecord(ctx->evEnd, st));
  record_backward(ctx, false);
  return RAU_OK;
}

// The loss terms an entry point was called with, normalised once: finite weights, named after `fn` (hop_w too, but
// for rau_backward and rau_graph_step, which take it as it is: check_hop_w); a term without a non-zero entry
// becomes null; a non-zero att_w needs the batch's targets; the scratch of every term left exists on return.
static int step_loss(rau_ctx* ctx, const char* fn, bool check_hop_w, const float* hop_w, const float* select_w,
                     const float* att_w, const float* merge_w, StepLoss* loss, const rau_out_grads* g = nullptr,
                     const rau_state_grads* sg = nullptr) {
  NEED(ctx && hop_w, "null argument");
  // the external record: all-null is absent (the caller's call then IS the one without it)
  rau_out_grads ext{nullptr, nullptr, nullptr};
  if (g) ext = *g;
  const bool has_ext = ext.d_logits || ext.d_dopred || ext.d_attprob;
  NEED((reinterpret_cast<uintptr_t>(ext.d_logits) & 15u) == 0, "%s: d_logits must be 16-byte aligned", fn);
  rau_state_grads sgr{nullptr, nullptr};
  if (sg) sgr = *sg;
  NEED(((reinterpret_cast<uintptr_t>(sgr.d_h) | reinterpret_cast<uintptr_t>(sgr.d_c_last)) & 15u) == 0,
       "%s: d_h and d_c_last must be 16-byte aligned", fn);
  const bool has_sg = sgr.d_h || sgr.d_c_last;
  if (merge_w) {
    NEED(std::isfinite(merge_w[0]) && std::isfinite(merge_w[1]), "%s: merge_w is not finite", fn);
    if (merge_w[0] == 0.f && merge_w[1] == 0.f) merge_w = nullptr;
    // the merged rows' terms are cross-entropies (merge_grad.hip): not part of a step trained with RAU_LOSS_BCE
    NEED(!merge_w || ctx->answer_loss == RAU_LOSS_CE,
         "%s: a non-zero merge_w under RAU_LOSS_BCE (rau_set_answer_loss): the merged rows are trained with the "
         "softmax cross-entropy only", fn);
    // ... and over the whole vocabulary: not part of a step whose criterion is restricted to candidates
    NEED(!merge_w || cur_batch(ctx).held.cand_C == 0,
         "%s: a non-zero merge_w on a batch with candidates (rau_set_candidates): the merged rows are trained with "
         "the full-vocabulary cross-entropy only", fn);
  }
  const int H = ctx->cfg.H;
  bool any = false, any_att = false, hop_any = false;
  int active = 0;
  for (int h = 0; h < H; ++h) {
    hop_any = hop_any || hop_w[h] != 0.f;
    NEED(!check_hop_w || std::isfinite(hop_w[h]), "%s: hop_w[%d] is not finite", fn, h);
    NEED(!select_w || std::isfinite(select_w[h]), "%s: select_w[%d] is not finite", fn, h);
    NEED(!att_w || std::isfinite(att_w[h]), "%s: att_w[%d] is not finite", fn, h);
    any = any || (select_w && select_w[h] != 0.f);
    any_att = any_att || (att_w && att_w[h] != 0.f);
    if (hop_w[h] != 0.f || (select_w && select_w[h] != 0.f) || (att_w && att_w[h] != 0.f)) active = h + 1;
  }
  if (any_att && !cur_batch(ctx).held.att_targets)
    return fail(RAU_ERR_STATE, "%s: a non-zero att_w needs a batch with attention targets (rau_set_att_targets)", fn);
  if (any_att || ext.d_attprob) {
    if (!ctx->att_da)   // sized for the capacity, cleared by rau_set_batch_size like every activation
      if (int rc = dalloc(ctx, &ctx->att_da, (size_t)H * ctx->cap * ctx->Sp)) return rc;
  }
  if ((any || ext.d_dopred) && !ctx->sel_add) {   // sized for the capacity, cleared by rau_set_batch_size like every activation
    if (!ctx->sel_s)
      if (int rc = dalloc(ctx, &ctx->sel_s, (size_t)H * ctx->cap)) return rc;
    if (int rc = dalloc(ctx, &ctx->sel_add, (size_t)H * ctx->cap * ctx->cfg.M)) return rc;
  }
  *loss = StepLoss{hop_w, any ? select_w : nullptr, any_att ? att_w : nullptr, merge_w,
                   (merge_w || has_ext || has_sg) ? H : active, ext, hop_any, sgr};
  return RAU_OK;
}

int rau_backward(rau_ctx* ctx, const float* hop_w) {
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_backward", false, hop_w, nullptr, nullptr, nullptr, &loss)) return rc;
  return backward_impl(ctx, loss);
}
int rau_backward_select(rau_ctx* ctx, const float* hop_w, const float* select_w) {
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_backward_select", true, hop_w, select_w, nullptr, nullptr, &loss)) return rc;
  return backward_impl(ctx, loss);
}
int rau_backward_att(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w) {
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_backward_att", true, hop_w, select_w, att_w, nullptr, &loss)) return rc;
  return backward_impl(ctx, loss);
}
int rau_backward_merged(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                        const float* merge_w) {
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_backward_merged", true, hop_w, select_w, att_w, merge_w, &loss)) return rc;
  return backward_impl(ctx, loss);
}
// The same with caller-supplied gradients at the three outputs (StepLoss::ext).  hop_w may be null (zeros) here: an
// external-only backward needs no label.  g null or all-null: rau_backward_merged, launch for launch.
int rau_backward_ext(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                     const float* merge_w, const rau_out_grads* g) {
  NEED(ctx, "null ctx");
  const bool has_ext = g && (g->d_logits || g->d_dopred || g->d_attprob);
  NEED(hop_w || has_ext, "rau_backward_ext: hop_w may be NULL only with a gradient in g");
  const std::vector<float> zeros((size_t)ctx->cfg.H, 0.f);
  StepLoss loss;
  if (int rc = step_loss(ctx, has_ext ? "rau_backward_ext" : "rau_backward_merged", true,
                         hop_w ? hop_w : zeros.data(), select_w, att_w, merge_w, &loss, g))
    return rc;
  return backward_impl(ctx, loss);   // (the staging copy of hop_w is taken before it returns)
}
// The same with caller-supplied gradients at the hop states (StepLoss::sg): d_h joins every hop's cell backward as its
// dh_next, d_c_last opens the recurrence.  sg null or all-null: rau_backward_ext, launch for launch.
int rau_backward_state(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                       const float* merge_w, const rau_out_grads* g, const rau_state_grads* sg) {
  NEED(ctx, "null ctx");
  if (!sg || !(sg->d_h || sg->d_c_last)) return rau_backward_ext(ctx, hop_w, select_w, att_w, merge_w, g);
  const std::vector<float> zeros((size_t)ctx->cfg.H, 0.f);
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_backward_state", true, hop_w ? hop_w : zeros.data(), select_w, att_w, merge_w,
                         &loss, g, sg))
    return rc;
  return backward_impl(ctx, loss);   // (the staging copy of hop_w is taken before it returns)
}
// Device pointers to c' / h' of every hop of the last step-level forward: rows [H][n][R] behind the initial-state rows
int rau_state_dev(rau_ctx* ctx, const float** c, const float** h) {
  NEED(ctx, "null ctx");
  if (!ctx->mg.valid)
    return fail(RAU_ERR_STATE, "rau_state_dev: no step-level forward to read (call rau_forward first)");
  const size_t BR_ = (size_t)ctx->cfg.B * ctx->cfg.R;
  if (c) *c = ctx->cc + BR_;
  if (h) *h = ctx->hh + BR_;
  return RAU_OK;
}
// Device pointers to the outputs of the last step-level forward, for a caller that computes its own gradients on
// the device.  Nothing is synchronised: the values are ordered on the ctx's stream.
int rau_outputs_dev(rau_ctx* ctx, const float** logits, const float** dopred, const float** attprob,
                    int32_t* att_pitch) {
  NEED(ctx, "null ctx");
  if (!ctx->mg.valid)
    return fail(RAU_ERR_STATE, "rau_outputs_dev: no step-level forward to read (call rau_forward first)");
  if (logits) *logits = ctx->logits;
  if (dopred) *dopred = ctx->dopred;
  if (attprob) *attprob = ctx->a;
  if (att_pitch) *att_pitch = ctx->Sp;
  return RAU_OK;
}
int rau_logits_pitch(rau_ctx* ctx, int32_t* pitch) {
  NEED(ctx && pitch, "rau_logits_pitch: null argument");
  *pitch = ctx->Kp;
  return RAU_OK;
}

// One training step's forward + backward (optionally with the gradient zeroing in front) as ONE
// hipGraph launch.  The three streams, their fork/join events and every kernel argument are
// captured once per step "shape" -- (mode, longest question, active hops, which mask sites are
// explicit, zeroing or not) -- and replayed; what changes from step to step lives in device
// memory: the batch (rau_set_batch), the Philox key (rau_set_dropout_seed) and the hop weights
// (uploaded here, in front of the launch).
// The weights are read from device memory, so they may change between replays; which terms have a non-zero one
// decides the launches and joins the key (StepKey), with the active-hop count.
static int graph_step_impl(rau_ctx* ctx, const StepLoss& loss, int zero_grads_first) {
  const BatchSlot& bs = cur_batch(ctx);
  if (!bs.held.have || !bs.held.have_labels)
    return fail(RAU_ERR_STATE, "rau_graph_step: needs a batch with labels (rau_set_batch)");
  if (ctx->prof_on) return fail(RAU_ERR_STATE, "rau_graph_step: profiling must be off");
  if (ctx->feat_grad && bs.held.n_images > 0 && !xgrad_per_image(ctx))
    return fail(RAU_ERR_STATE, "rau_graph_step: the feature-map gradient (rau_set_feat_grad) of a batch with an image "
                "table or bank rows is not formed; expand the maps per sample (rau_set_batch_dev)");
  const StepKey key = step_key(ctx, loss, zero_grads_first != 0);
  if (int rc = upload_hop_weights(ctx, loss)) return rc;
  ctx->mg.valid = false;
  hipGraphExec_t exec = nullptr;
  for (auto& g : ctx->graphs)
    if (g.key == key) exec = g.exec;
  if (!exec) {
    hipGraph_t graph = nullptr;
    HIPC(hipStreamBeginCapture(ctx->st, hipStreamCaptureModeRelaxed));
    ctx->capturing = true;
    int rc = zero_grads_first ? rau_zero_grads(ctx) : 0;
    if (!rc) rc = forward_impl(ctx, loss.forms_dpre());   // such a backward forms dpre / dhn itself
    if (!rc) rc = backward_impl(ctx, loss);
    ctx->capturing = false;
    hipError_t e = hipStreamEndCapture(ctx->st, &graph);
    if (rc) {
      if (graph) hipGraphDestroy(graph);
      return rc;
    }
    if (e != hipSuccess)
      return fail(RAU_ERR_DEVICE, "hipStreamEndCapture: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess)
      return fail(RAU_ERR_DEVICE, "hipGraphInstantiate: %s", hipGetErrorString(e));
    ctx->graphs.push_back({key, exec});
  }
  HIPC(hipGraphLaunch(exec, ctx->st));
  if (bs.held.n_images) {   // the graph's gather node has just filled feats_x from this upload
    ctx->x_valid = true;
    ctx->x_slot = ctx->cur_slot;
    ctx->x_serial = ctx->slot_serial[ctx->cur_slot];
  }
  HIPC(hipEventRecord(ctx->evEnd, ctx->st));   // a real (non-captured) end-of-step event
  ctx->fwd.xn_rows = ctx->xnorm ? ctx->cfg.B : 0;   // (a captured forward normalises the gathered per-sample maps)
  merge_record(ctx);
  drop_forward(ctx);
  record_backward(ctx, true);
  return RAU_OK;
}

int rau_graph_step(rau_ctx* ctx, const float* hop_w, int zero_grads_first) {
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_graph_step", false, hop_w, nullptr, nullptr, nullptr, &loss)) return rc;
  return graph_step_impl(ctx, loss, zero_grads_first);
}
int rau_graph_step_select(rau_ctx* ctx, const float* hop_w, const float* select_w, int zero_grads_first) {
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_graph_step_select", true, hop_w, select_w, nullptr, nullptr, &loss)) return rc;
  return graph_step_impl(ctx, loss, zero_grads_first);
}
int rau_graph_step_att(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                       int zero_grads_first) {
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_graph_step_att", true, hop_w, select_w, att_w, nullptr, &loss)) return rc;
  return graph_step_impl(ctx, loss, zero_grads_first);
}
int rau_graph_step_merged(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                          const float* merge_w, int zero_grads_first) {
  StepLoss loss;
  if (int rc = step_loss(ctx, "rau_graph_step_merged", true, hop_w, select_w, att_w, merge_w, &loss)) return rc;
  return graph_step_impl(ctx, loss, zero_grads_first);
}

int rau_wait_grads(rau_ctx* ctx, int group, void* hip_stream) {
  if (int rc = check_group(ctx, group)) return rc;
  if (!ctx->bwd.done) return fail(RAU_ERR_STATE, "rau_wait_grads: no rau_backward to wait for");
  hipStream_t s = (hipStream_t)hip_stream;
  if (group == RAU_GROUP_MULT && !ctx->bwd.graph) {
    // final once the bulk stream's conv gradients (evD) and the weight-gradient stream's
    // mult block (evM3) are done -- i.e. before the encoder BPTT, which they overlap
    HIPC(hipStreamWaitEvent(s, ctx->evD, 0));
    HIPC(hipStreamWaitEvent(s, ctx->evM3, 0));
  } else {
    HIPC(hipStreamWaitEvent(s, ctx->evEnd, 0));
  }
  return RAU_OK;
}

// ================================================================ results
// The persistent encoder's error word, read after a host synchronisation of the ctx stream: a bounded
// wait on a sibling workgroup's progress counter gave up (its siblings were not all resident: another
// process or context held the CUs).  THAT step's results are invalid and the call says so -- once:
// the word is cleared and the ctx falls back to the launch-per-step encoder for the rest of its life,
// so repeating the step succeeds instead of failing forever.
int persist_check(rau_ctx* ctx) {
  if (!(ctx->persist_used && ctx->perr_h && *ctx->perr_h)) return RAU_OK;
  *ctx->perr_h = 0;
  hipMemsetAsync(ctx->perr_d, 0, sizeof(int), ctx->st);
  hipStreamSynchronize(ctx->st);
  ctx->enc_ws = ctx->enc_ws_train = false;
  ctx->persist_gave_up = true;
  ctx->persist_used = false;
  drop_forward(ctx);
  ctx->mg.valid = false;
  return fail(RAU_ERR_DEVICE, "persistent encoder: a bounded wait on another workgroup's progress counter gave up; "
                              "the results of that step are invalid -- repeat it: this context now uses the "
                              "launch-per-step encoder");
}
int rau_sync(rau_ctx* ctx) {
  NEED(ctx, "null ctx");
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);
}
int d2h(rau_ctx* ctx, void* host, const void* dev, size_t bytes) {
  NEED(ctx && host, "null argument");
  HIPC(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);   // same check as rau_sync: never hand back such results as OK
}
int rau_get_losses(rau_ctx* ctx, float* losses) {
  NEED(ctx, "null ctx");
  return d2h(ctx, losses, ctx->losses_d, ctx->cfg.H * sizeof(float));
}
// The per-sample loss rows the losses are the means of (with sample weights: the weighted rows), dense [H, n]
int rau_get_loss_rows(rau_ctx* ctx, float* rows) {
  NEED(ctx && rows, "null argument");
  if (!ctx->mg.valid || !ctx->mg.truth.present())
    return fail(RAU_ERR_STATE, "rau_get_loss_rows: no step-level forward on a batch with a ground truth has left its "
                "loss rows (none has run yet, it failed, or a module-level entry point has run since)");
  return d2h(ctx, rows, ctx->lossrow, (size_t)ctx->cfg.H * ctx->cfg.B * sizeof(float));
}
int rau_get_argmax(rau_ctx* ctx, int32_t* ans) {
  NEED(ctx, "null ctx");
  return d2h(ctx, ans, ctx->argmax_d, (size_t)ctx->cfg.H * ctx->cfg.B * 4);
}
int rau_get_logits(rau_ctx* ctx, float* logits) {
  NEED(ctx, "null ctx");
  NEED(logits, "null argument");
  const rau_config& c = ctx->cfg;   // dense [H,n,K] on the host, rows at the answer pitch on the device
  if (ctx->Kp == c.K) return d2h(ctx, logits, ctx->logits, (size_t)c.H * c.B * c.K * 4);
  HIPC(hipMemcpy2DAsync(logits, (size_t)c.K * 4, ctx->logits, (size_t)ctx->Kp * 4, (size_t)c.K * 4, (size_t)c.H * c.B,
                        hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);
}
int rau_get_dopred(rau_ctx* ctx, float* dopred) {
  NEED(ctx, "null ctx");
  return d2h(ctx, dopred, ctx->dopred, (size_t)ctx->cfg.H * ctx->cfg.B * 4);
}
int rau_get_attention(rau_ctx* ctx, float* att) {
  NEED(ctx, "null ctx");
  NEED(att, "null argument");
  HIPC(hipMemcpy2DAsync(att, (size_t)ctx->cfg.S * 4, ctx->a, (size_t)ctx->Sp * 4,
                        (size_t)ctx->cfg.S * 4, (size_t)ctx->cfg.H * ctx->cfg.B,
                        hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return RAU_OK;
}
int rau_get_question_state(rau_ctx* ctx, float* q) {
  NEED(ctx, "null ctx");
  return d2h(ctx, q, question_state(ctx), (size_t)ctx->cfg.B * ctx->Q * 4);
}
int rau_get_att_state(rau_ctx* ctx, float* c, float* h) {
  NEED(ctx, "null ctx");
  const size_t BR_ = (size_t)ctx->cfg.B * ctx->cfg.R, n = (size_t)ctx->cfg.H * BR_;
  if (c)
    if (int rc = d2h(ctx, c, ctx->cc + BR_, n * 4)) return rc;
  if (h)
    if (int rc = d2h(ctx, h, ctx->hh + BR_, n * 4)) return rc;
  return RAU_OK;
}

// ================================================================= update
int rau_noise_clip_adam(rau_ctx* ctx, int64_t step_t, float lr, float mult_lr, float beta1,
                        float beta2, float eps, float eta, float gamma, float clip,
                        uint64_t noise_seed, float* out_norms) {
  NEED(ctx, "null ctx");
  NEED(step_t >= 0 && gamma > 0.f && eta >= 0.f && clip > 0.f, "bad update hyper-parameters");
  if (ctx->ema_swapped)   // reachable only through rau_ema_swap
    return fail(RAU_ERR_STATE, "rau_noise_clip_adam: the weights are swapped with their average (rau_ema_swap); "
                "swap back first");
  for (int gi = 0; gi < 3; ++gi)   // the state belongs to the rule that last wrote it (rau_update)
    if (ctx->grp[gi].adam_t > 0 && ctx->grp[gi].opt_rule != RAU_OPT_ADAM)
      return fail(RAU_ERR_STATE, "rau_noise_clip_adam: group %d holds Adamax state (t = %lld); reset it with "
                  "rau_set_opt_state first", gi, (long long)ctx->grp[gi].adam_t);
  if (int rc = update_guard(ctx, false, out_norms, 3)) return rc < 0 ? rc : RAU_OK;   // rau_set_update_guard
  hipStream_t st = ctx->st;
  // SS:598-599: var = eta / ((step_t+1) * gamma)
  const float nstd = eta > 0.f ? std::sqrt(eta / ((float)(step_t + 1) * gamma)) : 0.f;
  for (int gi = 0; gi < 3; ++gi) {
    Group& g = ctx->grp[gi];
    if (!g.m) {
      if (int rc = dalloc(ctx, &g.m, g.n, false)) return rc;
      if (int rc = dalloc(ctx, &g.v, g.n, false)) return rc;
    }
    g.adam_t += 1;
    g.opt_rule = RAU_OPT_ADAM;
    const double bc1 = 1.0 - std::pow((double)beta1, (double)g.adam_t);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)g.adam_t);
    const float group_lr = gi == RAU_GROUP_MULT ? mult_lr : lr;  // SS:770-772
    const float stepsize = (float)(group_lr * std::sqrt(bc2) / bc1);
    RUN("noise_sqnorm", 0, g.n * 8.0,
        add_noise_sqnorm(st, g.n, g.g, nstd, noise_seed + (uint64_t)step_t * 3 + gi, (uint32_t)gi,
                         ctx->npart));
    RUN("finish_norm", 0, 0, finish_norm(st, 1024, ctx->npart, ctx->norms_d + gi));
    RUN("clip_adam", 0, g.n * 28.0,
        clip_adam(st, g.n, g.w, g.g, g.m, g.v, ctx->norms_d + gi, clip, stepsize, beta1, beta2, eps));
  }
  if (out_norms) return d2h(ctx, out_norms, ctx->norms_d, 3 * sizeof(float));
  return RAU_OK;
}

// ================================================================= timing
int rau_stream(rau_ctx* ctx, void** hip_stream) {
  NEED(ctx && hip_stream, "null argument");
  *hip_stream = (void*)ctx->st;
  return RAU_OK;
}
int rau_timer_begin(rau_ctx* ctx) {
  NEED(ctx, "null ctx");
  HIPC(hipEventRecord(ctx->ev0, ctx->st));
  return RAU_OK;
}
int rau_timer_end(rau_ctx* ctx, float* ms) {
  NEED(ctx && ms, "null argument");
  HIPC(hipEventRecord(ctx->ev1, ctx->st));
  HIPC(hipEventSynchronize(ctx->ev1));
  HIPC(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
  return RAU_OK;
}
int rau_prof_enable(rau_ctx* ctx, int on) {
  NEED(ctx, "null ctx");
  if (!on)
    if (int rc = prof_collect(ctx)) return rc;
  ctx->prof_on = on != 0;
  ctx->prof_sparse = on == 2;
  return RAU_OK;
}
int rau_prof_reset(rau_ctx* ctx) {
  NEED(ctx, "null ctx");
  if (int rc = prof_collect(ctx)) return rc;
  ctx->pcls.clear();
  return RAU_OK;
}
int rau_prof_count(rau_ctx* ctx) {
  if (!ctx) return fail(RAU_ERR_INVALID, "null ctx");
  if (int rc = prof_collect(ctx)) return rc;
  return (int)ctx->pcls.size();
}
int rau_prof_entry(rau_ctx* ctx, int index, const char** name, int64_t* launches, double* total_ms,
                   double* flops, double* bytes) {
  NEED(ctx, "null ctx");
  NEED(index >= 0 && index < (int)ctx->pcls.size(), "prof index %d out of range", index);
  const ProfCls& p = ctx->pcls[index];
  if (name) *name = p.name.c_str();
  if (launches) *launches = p.launches;
  if (total_ms) *total_ms = p.ms;
  if (flops) *flops = p.flops;
  if (bytes) *bytes = p.bytes;
  return RAU_OK;
}

}  // extern "C"

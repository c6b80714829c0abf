--[[ rau.lua -- LuaJIT FFI shim over librau.so (include/rau.h).

Presents the reference's nn.Module call surface for the RAU hot path so that
experiments/Ours_*/LstmAttCtrlGradNoiseDontSelect.lua keeps its structure:
  :training() / :evaluate()          (SS:449-450, 479, 648-649, 676)
  :getParameters()                   (SS:322-324)  -> flat param / grad handles
  feval's tensor half                (SS:428-596)  -> rau:forward() / rau:backward(w, select_w, att_w)
  adam(x, dx, lr, ...) x 3 + noise + clip (SS:597-630, 770-772) -> rau:update(...)

No LuaJIT/Torch7 toolchain exists in the build image, so this file is shipped as
source and is NOT exercised by the tests; the Python ctypes binding
(rau_vqa_amd/_lib.py) is the executable proof of the identical ABI.
INTEGRATION.md shows the reference-side patch that uses this file.
]]
local ffi = require 'ffi'

ffi.cdef[[
typedef struct rau_config {
  int32_t B, T, V, E, Rq, D, S, M, A, R, K, H;
  float p_we, p_rnn, p_q, p_x, p_mf;
  int32_t dtype, device_id;
} rau_config;
typedef struct rau_ctx rau_ctx;
void rau_default_config(rau_config* cfg);
const char* rau_last_error(void);
int rau_abi_version(void);
int rau_create(const rau_config* cfg, rau_ctx** out);
void rau_destroy(rau_ctx* ctx);
int rau_set_batch_size(rau_ctx* ctx, int32_t n);
int rau_batch_size(rau_ctx* ctx, int32_t* n, int32_t* capacity);
int rau_params(rau_ctx* ctx, int group, float** weights, float** grads, size_t* n);
int rau_layout_count(const rau_ctx* ctx, int group);
int rau_layout_entry(const rau_ctx* ctx, int group, int index, const char** name,
                     size_t* offset, int32_t* rows, int32_t* cols);
int rau_set_params(rau_ctx* ctx, int group, const float* host, size_t n);
int rau_get_params(rau_ctx* ctx, int group, float* host, size_t n);
int rau_get_grads(rau_ctx* ctx, int group, float* host, size_t n);
int rau_set_grads(rau_ctx* ctx, int group, const float* host, size_t n);
int rau_init_uniform(rau_ctx* ctx, uint64_t seed, float lo, float hi);
int rau_zero_grads(rau_ctx* ctx);
int rau_set_mode(rau_ctx* ctx, int mode);
int rau_set_dropout_seed(rau_ctx* ctx, uint64_t seed, uint32_t step);
int rau_set_mask(rau_ctx* ctx, int site, const uint8_t* keep, size_t n);
int rau_get_mask(rau_ctx* ctx, int site, uint8_t* keep, size_t n);
int rau_set_feat_dropout(rau_ctx* ctx, int kind);
int rau_feat_dropout(rau_ctx* ctx, int* kind);
int rau_set_answer_loss(rau_ctx* ctx, int kind);
int rau_answer_loss(rau_ctx* ctx, int* kind);
int rau_set_batch(rau_ctx* ctx, const float* feats, const int32_t* tokens,
                  const int32_t* lens, const int32_t* labels);
int rau_batch_feats(rau_ctx* ctx, float** feats_dev);
int rau_set_batch_typed(rau_ctx* ctx, const void* feats, int feat_type, const int32_t* tokens,
                        const int32_t* lens, const int32_t* labels);
int rau_set_batch_async_typed(rau_ctx* ctx, int slot, const void* feats, int feat_type,
                              const int32_t* tokens, const int32_t* lens, const int32_t* labels,
                              int has_labels);
int rau_batch_feat_type(rau_ctx* ctx, int* feat_type);
int rau_set_batch_images(rau_ctx* ctx, const void* feats, int feat_type, int n_images,
                         const int32_t* image_of, const int32_t* tokens, const int32_t* lens,
                         const int32_t* labels);
int rau_set_batch_async_images(rau_ctx* ctx, int slot, const void* feats, int feat_type, int n_images,
                               const int32_t* image_of, const int32_t* tokens, const int32_t* lens,
                               const int32_t* labels, int has_labels);
int rau_batch_images(rau_ctx* ctx, int* n_images);
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
int rau_batch_slot(rau_ctx* ctx, int slot, float** feats_host, int32_t** tokens_host,
                   int32_t** lens_host, int32_t** labels_host);
int rau_set_batch_async(rau_ctx* ctx, int slot, const float* feats, const int32_t* tokens,
                        const int32_t* lens, const int32_t* labels, int has_labels);
int rau_use_batch(rau_ctx* ctx, int slot);
int rau_set_answers(rau_ctx* ctx, int slot, int32_t G, const int32_t* ids, const float* w,
                    const float* score);
int rau_batch_answers(rau_ctx* ctx, int32_t* G);
int rau_set_regions(rau_ctx* ctx, int slot, const int32_t* n);
int rau_batch_regions(rau_ctx* ctx, int* has);
int rau_set_sample_weights(rau_ctx* ctx, int slot, const float* s);
int rau_batch_sample_weights(rau_ctx* ctx, int* has);
int rau_set_candidates(rau_ctx* ctx, int slot, int32_t C, const int32_t* cand);
int rau_batch_candidates(rau_ctx* ctx, int32_t* C);
int rau_set_batch_packed(rau_ctx* ctx, const void* rows, int feat_type, int n_maps, const int32_t* counts,
                         const int32_t* image_of, const int32_t* tokens, const int32_t* lens,
                         const int32_t* labels);
int rau_set_batch_async_packed(rau_ctx* ctx, int slot, const void* rows, int feat_type, int n_maps,
                               const int32_t* counts, const int32_t* image_of, const int32_t* tokens,
                               const int32_t* lens, const int32_t* labels, int has_labels);
int rau_bank_put_packed(rau_ctx* ctx, int32_t first, int32_t count, const void* rows, int src_type,
                        const int32_t* counts);
int rau_forward(rau_ctx* ctx);
int rau_backward(rau_ctx* ctx, const float* hop_w);
int rau_backward_select(rau_ctx* ctx, const float* hop_w, const float* select_w);
int rau_graph_step_select(rau_ctx* ctx, const float* hop_w, const float* select_w, int zero_grads_first);
int rau_set_att_targets(rau_ctx* ctx, int slot, const float* t);
int rau_batch_att_targets(rau_ctx* ctx, int* has);
int rau_backward_att(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w);
int rau_graph_step_att(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w, int zero_grads_first);
int rau_att_stats(rau_ctx* ctx, float* loss, float* mass, int32_t* hits, int32_t* n_sup);
int rau_backward_merged(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                        const float* merge_w);
int rau_graph_step_merged(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                          const float* merge_w, int zero_grads_first);
int rau_merge_criterion_backward(rau_ctx* ctx, const float* logits_dev, const float* dopred_dev,
                                 const int32_t* labels_dev, const float* merge_w, float* d_logits_dev);
typedef struct rau_out_grads {
  const float* d_logits;
  const float* d_dopred;
  const float* d_attprob;
} rau_out_grads;
int rau_set_feat_grad(rau_ctx* ctx, int on);
int rau_feat_grad(rau_ctx* ctx, int* on);
int rau_feat_grad_dev(rau_ctx* ctx, const float** dX, int32_t* pitch);
int rau_feat_grad_rows(rau_ctx* ctx, int32_t* rows);
int rau_get_feat_grad(rau_ctx* ctx, float* host);
int rau_set_feat_norm(rau_ctx* ctx, int kind, float eps);
int rau_feat_norm(rau_ctx* ctx, int* kind, float* eps);
int rau_norm_feats_dev(rau_ctx* ctx, const float** xn, const float** nrm, int32_t* pitch, int32_t* rows);
int rau_get_norm_feats(rau_ctx* ctx, float* xn_host, float* nrm_host);
int rau_set_batch_dev(rau_ctx* ctx, const float* feats_dev, const int32_t* tokens, const int32_t* lens, const int32_t* labels);
int rau_set_question_dev(rau_ctx* ctx, const void* q_dev, int q_type);
int rau_batch_question(rau_ctx* ctx, int* has);
int rau_question_grad_dev(rau_ctx* ctx, const float** dq);
int rau_get_question_grad(rau_ctx* ctx, float* host);
int rau_set_batch_dev_images(rau_ctx* ctx, const float* table_dev, int n_images, const int32_t* image_of,
                             const int32_t* tokens, const int32_t* lens, const int32_t* labels);
int rau_outputs_dev(rau_ctx* ctx, const float** logits, const float** dopred, const float** attprob,
                    int32_t* att_pitch);
int rau_logits_pitch(rau_ctx* ctx, int32_t* pitch);
int rau_backward_ext(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                     const float* merge_w, const rau_out_grads* g);
int rau_set_state_dev(rau_ctx* ctx, const void* c0_dev, const void* h0_dev, int type);
int rau_batch_state(rau_ctx* ctx, int* has);
int rau_state_dev(rau_ctx* ctx, const float** c, const float** h);
typedef struct rau_state_grads {
  const float* d_h;
  const float* d_c_last;
} rau_state_grads;
int rau_backward_state(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                       const float* merge_w, const rau_out_grads* g, const rau_state_grads* sg);
int rau_state_grad_dev(rau_ctx* ctx, const float** d_c0, const float** d_h0);
int rau_get_state_grad(rau_ctx* ctx, float* d_c0_host, float* d_h0_host);
int rau_set_att_bias_dev(rau_ctx* ctx, const void* bias_dev, int type);
int rau_batch_att_bias(rau_ctx* ctx, int* has);
int rau_att_bias_grad_dev(rau_ctx* ctx, const float** d_bias, int32_t* pitch);
int rau_get_att_bias_grad(rau_ctx* ctx, float* host);
int rau_embed_forward(rau_ctx* ctx, int t, const int32_t* tokens_dev, float** we);
int rau_embed_backward(rau_ctx* ctx, int t, const int32_t* tokens_dev, const float* d_we);
int rau_deeplstm_forward(rau_ctx* ctx, int t, const float* x, const float* state,
                         float** state_out);
int rau_deeplstm_backward(rau_ctx* ctx, int t, const float* x, const float* state,
                          const float* d_state_out, float** d_x, float** d_state);
int rau_multimodal_forward(rau_ctx* ctx, int h, const float* q, const float* X,
                           const float* c_prev, const float* h_prev, float** logits,
                           float** do_pred, float** attprob, float** c_out, float** h_out);
int rau_multimodal_forward_regions(rau_ctx* ctx, int h, const float* q, const float* X,
                                   const float* c_prev, const float* h_prev, const int32_t* regions_dev,
                                   float** logits, float** do_pred, float** attprob, float** c_out,
                                   float** h_out);
int rau_multimodal_forward_bias(rau_ctx* ctx, int h, const float* q, const float* X,
                                const float* c_prev, const float* h_prev, const int32_t* regions_dev,
                                const float* bias_dev, float** logits, float** do_pred, float** attprob,
                                float** c_out, float** h_out);
int rau_multimodal_backward(rau_ctx* ctx, int h, const float* q, const float* X,
                            const float* c_prev, const float* h_prev, const float* d_logits,
                            const float* d_do_pred, const float* d_attprob,
                            const float* d_c, const float* d_h, float** d_q, float** d_X,
                            float** d_c_prev, float** d_h_prev);
int rau_criterion_forward(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev,
                          float* loss);
int rau_criterion_backward(rau_ctx* ctx, int h, const float* logits,
                           const int32_t* labels_dev, float scale, float** d_logits);
int rau_criterion_forward_set(rau_ctx* ctx, int h, const float* logits, int32_t G, const int32_t* ids_dev,
                              const float* w_dev, float* loss);
int rau_criterion_backward_set(rau_ctx* ctx, int h, const float* logits, int32_t G, const int32_t* ids_dev,
                               const float* w_dev, float scale, float** d_logits);
int rau_criterion_forward_bce(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev,
                              int32_t G, const int32_t* ids_dev, const float* w_dev, float* loss);
int rau_criterion_backward_bce(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev,
                               int32_t G, const int32_t* ids_dev, const float* w_dev, float scale, float** d_logits);
int rau_criterion_forward_cand(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev,
                               int32_t G, const int32_t* ids_dev, const float* w_dev, int32_t C, const int32_t* cand_dev,
                               int kind, float* loss);
int rau_criterion_backward_cand(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, int32_t G,
                                const int32_t* ids_dev, const float* w_dev, int32_t C, const int32_t* cand_dev, int kind,
                                float scale, float** d_logits);
int rau_att_criterion_forward(rau_ctx* ctx, int h, const float* attprob_dev, const float* t_dev,
                              const int32_t* nreg_dev, float* loss);
int rau_att_criterion_backward(rau_ctx* ctx, int h, const float* attprob_dev, const float* t_dev,
                               const int32_t* nreg_dev, float scale, float** d_attprob);
int rau_dev_alloc(rau_ctx* ctx, size_t n_floats, float** out);
int rau_dev_free(rau_ctx* ctx, float* p);
int rau_dev_fill(rau_ctx* ctx, float* dst, size_t n, float value);
int rau_dev_copy(rau_ctx* ctx, float* dst, const float* src, size_t n);
int rau_dev_axpy(rau_ctx* ctx, float* y, const float* x, size_t n, float alpha);
int rau_dev_scale(rau_ctx* ctx, float* x, size_t n, float alpha);
int rau_dev_addcmul(rau_ctx* ctx, float* y, float alpha, const float* x1, const float* x2, size_t n);
int rau_dev_addcdiv(rau_ctx* ctx, float* y, float alpha, const float* x1, const float* x2, size_t n);
int rau_dev_sqrt(rau_ctx* ctx, float* x, size_t n);
int rau_dev_add_scalar(rau_ctx* ctx, float* x, size_t n, float value);
int rau_dev_adam(rau_ctx* ctx, float* x, const float* dx, float* m, float* v, size_t n, float lr,
                 float beta1, float beta2, float eps, int32_t t);
int rau_dev_adamax(rau_ctx* ctx, float* x, const float* dx, float* m, float* u, size_t n, float lr,
                   float beta1, float beta2, float eps, int32_t t);
int rau_dev_scale_rows(rau_ctx* ctx, float* x, int32_t rows, int32_t cols, int32_t ld, const float* s_dev);
int rau_dev_l2norm(rau_ctx* ctx, const float* x_dev, int32_t n, float eps, float* y_dev, float* nrm_dev);
int rau_dev_l2norm_backward(rau_ctx* ctx, const float* y_dev, const float* nrm_dev, float eps, const float* g_dev, int32_t n, float* dx_dev);
int rau_dev_select_rows(rau_ctx* ctx, float* dst, const float* src, int32_t rows, int32_t cols,
                        const int32_t* key_dev, int32_t value);
int rau_dev_rowmax(rau_ctx* ctx, const float* x, int32_t rows, int32_t cols, float* max_dev,
                   int32_t* argmax_dev);
int rau_dev_topk(rau_ctx* ctx, const float* x, int32_t rows, int32_t cols, int32_t k,
                 float* val_dev, int32_t* idx_dev);
int rau_dev_sum(rau_ctx* ctx, const float* x, size_t n, double* out_host);
int rau_dev_count_eq(rau_ctx* ctx, const int32_t* a_dev, const int32_t* b_dev, int32_t n,
                     int32_t* count_host);
int rau_dev_upload(rau_ctx* ctx, void* dst_dev, const void* host, size_t bytes);
int rau_dev_download(rau_ctx* ctx, void* host, const void* src_dev, size_t bytes);
int rau_graph_step(rau_ctx* ctx, const float* hop_w, int zero_grads_first);
int rau_sync(rau_ctx* ctx);
int rau_get_losses(rau_ctx* ctx, float* losses);
int rau_get_loss_rows(rau_ctx* ctx, float* rows);
int rau_get_argmax(rau_ctx* ctx, int32_t* ans);
int rau_get_logits(rau_ctx* ctx, float* logits);
int rau_get_dopred(rau_ctx* ctx, float* dopred);
int rau_get_attention(rau_ctx* ctx, float* att);
int rau_get_question_state(rau_ctx* ctx, float* q);
int rau_get_att_state(rau_ctx* ctx, float* c, float* h);
int rau_step_stats(rau_ctx* ctx, float* loss, float* loss_do_pred, int32_t* counts);
int rau_step_scores(rau_ctx* ctx, float* per_sample, float* total);
int rau_predict_scores(rau_ctx* ctx, float* oe, float* mc, float* totals);
int rau_predict(rau_ctx* ctx, const int32_t* mc_ans, int32_t n_mc, int32_t* oe, int32_t* mc);
int rau_get_merged(rau_ctx* ctx, float* pred, float* att);
int rau_topk(rau_ctx* ctx, int32_t k, int32_t* ids, float* score, float* conf);
int rau_cand_stats(rau_ctx* ctx, float* loss, int32_t* correct, float* score, int32_t* n_lab);
int rau_topk_cand(rau_ctx* ctx, int32_t k, int32_t* ids, float* score, float* conf);
int rau_noise_clip_adam(rau_ctx* ctx, int64_t step_t, float lr, float mult_lr,
                        float beta1, float beta2, float eps, float eta, float gamma,
                        float clip, uint64_t noise_seed, float* out_norms);
typedef struct rau_update_opts {
  int32_t rule, clip_scope;
  float lr, mult_lr, beta1, beta2, eps, eta, gamma, clip;
  uint64_t noise_seed;
} rau_update_opts;
void rau_update_opts_default(rau_update_opts* o);
int rau_update(rau_ctx* ctx, int64_t step_t, const rau_update_opts* o, float* out_norms);
int rau_get_opt_state(rau_ctx* ctx, int group, float* m, float* v, int64_t* t, int32_t* rule);
int rau_set_opt_state(rau_ctx* ctx, int group, const float* m, const float* v, int64_t t, int32_t rule);
typedef struct rau_update_extras {
  float weight_decay;
  float ema_decay;
} rau_update_extras;
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
typedef struct rau_layer_stat {
  float sumsq[3];
  float absmax[3];
  int64_t nonfinite[3];
  int64_t n;
} rau_layer_stat;
int rau_layer_stats_count(const rau_ctx* ctx);
int rau_layer_stats(rau_ctx* ctx, int what, float eps, rau_layer_stat* out);
int rau_layer_stats_dev(rau_ctx* ctx, int what, float eps, const rau_layer_stat** dev);
int rau_set_update_guard(rau_ctx* ctx, int mode);
int rau_update_guard(rau_ctx* ctx, int* mode, int64_t* skipped, int32_t* last_skipped,
                     int64_t last_nonfinite[3]);
int rau_stream(rau_ctx* ctx, void** hip_stream);
int rau_wait_grads(rau_ctx* ctx, int group, void* hip_stream);
int rau_comm_unique_id(void* id, size_t bytes);
int rau_comm_init(rau_ctx* ctx, int nranks, int rank, const void* id, size_t bytes);
int rau_allreduce_grads(rau_ctx* ctx);
int rau_comm_destroy(rau_ctx* ctx);
int rau_timer_begin(rau_ctx* ctx);
int rau_timer_end(rau_ctx* ctx, float* ms);
int rau_prof_enable(rau_ctx* ctx, int on);
int rau_prof_reset(rau_ctx* ctx);
int rau_prof_count(rau_ctx* ctx);
int rau_prof_entry(rau_ctx* ctx, int index, const char** name, int64_t* launches,
                   double* total_ms, double* flops, double* bytes);
int rau_split_guard_check(size_t ws_floats, size_t offset, int nsplit, size_t per_split_floats);
int rau_image_lists(int n, int n_images, const int32_t* image_of, int32_t* start, int32_t* samples);
int rau_enc_ws_coresident(int batch, int blocks_per_cu, int n_cus);
]]

local C = ffi.load(os.getenv('RAU_LIB') or 'librau.so')
local GROUP = { embed = 0, rnn = 1, mult = 2 }

local function check(rc)
  if rc ~= 0 then error('librau: ' .. ffi.string(C.rau_last_error()), 3) end
end

local RAU = {}
RAU.__index = RAU

-- opt: the reference's hard-coded locals (SS:202-229) plus data-defined sizes
function RAU.new(opt)
  local cfg = ffi.new('rau_config[1]')
  C.rau_default_config(cfg)
  for k, v in pairs(opt) do cfg[0][k] = v end
  local h = ffi.new('rau_ctx*[1]')
  check(C.rau_create(cfg, h))
  -- `life.alive` is what device-tensor finalizers look at: the collector may run them after the
  -- context's own finalizer, and rau_destroy has then freed their memory already
  local life = { alive = true }
  local self = setmetatable({ h = ffi.gc(h[0], function(p) life.alive = false; C.rau_destroy(p) end),
                              cfg = cfg[0], life = life, scratch = {} }, RAU)
  self.n = self.cfg.B   -- current batch size (rau:setBatchSize); cfg.B stays the capacity
  return self
end

-- One context, batches of up to cfg.B rows: rau:setBatchSize(n) makes it behave, bit for bit, like a context
-- created with B = n that holds the same parameters, gradients, optimizer state, dropout seed, mode and bank
-- (the reference's test_* tensors of SS:387-410 on the training context).  The resident batch, both upload slots
-- and the last results do not outlive the call; it drains the streams and clears the activation storage, so
-- call it per epoch (train -> evaluate -> train), not per step.  rau:batchSize() -> current size, capacity.
function RAU:setBatchSize(n)
  if n < 1 or n > self.cfg.B then
    error(string.format('rau:setBatchSize(%d): out of [1, %d] (the batch size the context was created with)',
                        n, self.cfg.B), 2)
  end
  check(C.rau_set_batch_size(self.h, n))
  self.n = n
end
function RAU:batchSize()
  local n, cap = ffi.new('int32_t[1]'), ffi.new('int32_t[1]')
  check(C.rau_batch_size(self.h, n, cap))
  return n[0], cap[0]
end
-- the setBatch* family: a batch whose x_len has another row count than the current size switches first
local function follow_rows(self, x_len)
  if x_len and x_len:nElement() ~= self.n then self:setBatchSize(x_len:nElement()) end
end

-- nn.Module surface ----------------------------------------------------------
function RAU:training() check(C.rau_set_mode(self.h, 0)); return self end
function RAU:evaluate() check(C.rau_set_mode(self.h, 1)); return self end
-- One feature-map dropout mask for all hops (RAU_XDROP_TIED) instead of the reference's mask per hop clone: a
-- train-mode step then runs the two 1x1 convs and their gradients once.  on = false (or nil given as false)
-- goes back to the reference's masks.  Between steps; a change drops an explicit feature-map mask.
function RAU:tieFeatureDropout(on)
  check(C.rau_set_feat_dropout(self.h, (on == nil or on) and 1 or 0))
  return self
end
function RAU:featureDropoutTied()
  local k = ffi.new('int[1]')
  check(C.rau_feat_dropout(self.h, k))
  return k[0] == 1
end
-- The answer criterion of forward / graphStep: 'ce' (softmax cross-entropy, the reference's) or 'bce' (a sigmoid per
-- answer, binary cross-entropy against the soft targets of the answer set).  Between steps; a change drops the last
-- forward.  A non-zero merge_w is refused under 'bce'.
local LOSS = { ce = 0, bce = 1 }
function RAU:setAnswerLoss(kind)
  local k = LOSS[kind]
  if k == nil then error("setAnswerLoss: kind must be 'ce' or 'bce'") end
  check(C.rau_set_answer_loss(self.h, k))
  return self
end
function RAU:answerLoss()
  local k = ffi.new('int[1]')
  check(C.rau_answer_loss(self.h, k))
  return k[0] == 1 and 'bce' or 'ce'
end

-- m:getParameters(): returns {ptr=device float*, grad=device float*, n=count}
function RAU:getParameters(group)
  local w, g, n = ffi.new('float*[1]'), ffi.new('float*[1]'), ffi.new('size_t[1]')
  check(C.rau_params(self.h, GROUP[group], w, g, n))
  return { ptr = w[0], grad = g[0], n = tonumber(n[0]) }
end

-- param:uniform(-0.08, 0.08), SS:352-354
function RAU:reset(seed, lo, hi) check(C.rau_init_uniform(self.h, seed or 123, lo or -0.08, hi or 0.08)) end

-- feats: FloatTensor [B,D,W,H]; x: IntTensor [T,B]; x_len, y: IntTensor [B]  (loader.lua:1009)
-- A HalfTensor feats goes up as fp16 (rau_set_batch_typed): half the bytes, the same results
-- bit for bit as feats:float().
-- fp8 maps (OCP e4m3fn / e5m2, one byte per element) travel as a ByteTensor of bit patterns and must be
-- named: Torch7 has no fp8 tensor, so a ByteTensor without feat_type 'e4m3' | 'e5m2' is an error.
local FEAT = { f32 = 0, f16 = 1, bf16 = 2, e4m3 = 4, e5m2 = 5 }   -- rau_feat_type (3 is reserved)
local FEAT_BYTES = { f32 = 4, f16 = 2, bf16 = 2, e4m3 = 1, e5m2 = 1 }   -- bytes per element
-- the rau_feat_type a tensor stands for: `feat_type` if given, else from the tensor's type
local function feat_type_of(feats, feat_type)
  local ty = feats and torch.type(feats)
  if ty == 'torch.ByteTensor' then
    assert(feat_type == 'e4m3' or feat_type == 'e5m2', "a ByteTensor of features needs feat_type 'e4m3' or 'e5m2'")
  elseif feat_type == 'e4m3' or feat_type == 'e5m2' then
    assert(feats == nil, 'fp8 features are a ByteTensor of bit patterns')
  end
  local name = feat_type or (ty == 'torch.HalfTensor' and 'f16') or 'f32'
  return assert(FEAT[name], 'unknown feat_type ' .. tostring(name)), name
end
function RAU:setBatch(feats, x, x_len, y, feat_type)
  follow_rows(self, x_len)
  local ft = feat_type_of(feats, feat_type)
  if ft ~= FEAT.f32 then
    check(C.rau_set_batch_typed(self.h, feats:data(), ft, x:data(), x_len:data(), y and y:data() or nil))
  else
    check(C.rau_set_batch(self.h, feats:data(), x:data(), x_len:data(), y and y:data() or nil))
  end
end

-- Asynchronous, double-buffered upload (slot = 0 | 1): what SS:434-439 does every iteration, moved
-- behind the loader's prefetch.  rau:batchSlot(slot) returns host tensors OVER the slot's pinned
-- staging (torch storages on foreign memory: no copy, not owned) for next_batch_feat's worker to
-- assemble the batch in; rau:setBatchAsync(slot) enqueues the upload of what is in them (pass
-- tensors to have them copied into the staging first); rau:useBatch(slot) makes it the resident
-- batch -- the step's streams wait for the copies by an event, the host never does.
-- feat_type 'f16': the slot's feats come back as a HalfTensor over the start of its staging; 'e4m3' | 'e5m2':
-- as a ByteTensor (n bytes) over its start.
function RAU:batchSlot(slot, feat_type)
  local f, x, l, y = ffi.new('float*[1]'), ffi.new('int32_t*[1]'), ffi.new('int32_t*[1]'), ffi.new('int32_t*[1]')
  check(C.rau_batch_slot(self.h, slot, f, x, l, y))
  local c, B = self.cfg, self.n   -- each array starts where the capacity puts it and is dense in the current size
  local function addr(p) return tonumber(ffi.cast('intptr_t', p)) end
  local n = B * c.D * c.S
  return {
    feats = feat_type == 'f16' and torch.HalfTensor(torch.HalfStorage(n, addr(f[0]))):resize(B, c.D, c.S)
            or FEAT_BYTES[feat_type or 'f32'] == 1
               and torch.ByteTensor(torch.ByteStorage(n, addr(f[0]))):resize(B, c.D, c.S)
            or torch.FloatTensor(torch.FloatStorage(n, addr(f[0]))):resize(B, c.D, c.S),
    x = torch.IntTensor(torch.IntStorage(c.T * B, addr(x[0]))):resize(c.T, B),
    x_len = torch.IntTensor(torch.IntStorage(B, addr(l[0]))),
    y = torch.IntTensor(torch.IntStorage(B, addr(y[0]))),
  }
end
function RAU:setBatchAsync(slot, feats, x, x_len, y, has_labels, feat_type)
  follow_rows(self, x_len)
  local ft = feat_type_of(feats, feat_type)
  check(C.rau_set_batch_async_typed(self.h, slot, feats and feats:data() or nil, ft, x and x:data() or nil,
                                    x_len and x_len:data() or nil, y and y:data() or nil,
                                    (has_labels == false) and 0 or 1))
end
function RAU:useBatch(slot) check(C.rau_use_batch(self.h, slot)) end

-- Multi-answer ground truth (rau_set_answers): ids IntTensor [B,G] of 1-based answer ids (0 = empty entry), w
-- FloatTensor [B,G] of loss weights, score FloatTensor [B,G] of metric scores (nil: w), G <= 16.  slot = nil: the
-- resident batch (call it after setBatch); slot = 0 | 1: after setBatchAsync(slot, ...) and before useBatch(slot).
-- The set replaces y in the criterion head and in stepStats until the next batch goes into that slot.
function RAU:setAnswers(ids, w, score, slot)
  ids, w = ids:int():contiguous(), w:float():contiguous()
  score = score and score:float():contiguous()
  assert(ids:dim() == 2 and ids:size(1) == self.n and w:isSameSizeAs(ids), 'ids and w must be [B,G]')
  assert(not score or score:isSameSizeAs(ids), 'score must be [B,G]')
  check(C.rau_set_answers(self.h, slot or -1, ids:size(2), ids:data(), w:data(), score and score:data() or nil))
end
-- G of the resident batch's answer set, 0 without one
function RAU:batchAnswers()
  local g = ffi.new('int32_t[1]')
  check(C.rau_batch_answers(self.h, g))
  return g[0]
end

-- Region counts (rau_set_regions): n IntTensor [B], 1 <= n[b] <= S; sample b attends to its first n[b] positions
-- only (prefix-packed region features, padded grids), the others get attention and gradient exactly 0.  Always
-- per SAMPLE: for an image table gather it first, n_image:index(1, image_of:long()).  slot as in setAnswers; the
-- counts last until the next batch goes into that slot.
function RAU:setRegions(n, slot)
  n = n:int():contiguous()
  assert(n:dim() == 1 and n:size(1) == self.n, 'n must be [B]')
  check(C.rau_set_regions(self.h, slot or -1, n:data()))
end
-- whether the resident batch carries region counts
function RAU:batchRegions()
  local v = ffi.new('int[1]')
  check(C.rau_batch_regions(self.h, v))
  return v[0] ~= 0
end

-- Per-sample loss weights (rau_set_sample_weights): s FloatTensor [B], finite and >= 0; every built-in mean of the
-- step path, (1/n) sum_b row_b, becomes (1/n) sum_b s[b] row_b.  Never renormalised by the library.  nil detaches
-- them.  slot as in setAnswers; the weights last until the next batch goes into that slot.
function RAU:setSampleWeights(s, slot)
  if s == nil then
    check(C.rau_set_sample_weights(self.h, slot or -1, nil))
    return
  end
  s = s:float():contiguous()
  assert(s:dim() == 1 and s:size(1) == self.n, 's must be [B]')
  check(C.rau_set_sample_weights(self.h, slot or -1, s:data()))
end
-- whether the resident batch carries sample weights
function RAU:batchSampleWeights()
  local v = ffi.new('int[1]')
  check(C.rau_batch_sample_weights(self.h, v))
  return v[0] ~= 0
end
-- Multiple-choice candidates (rau_set_candidates): cand IntTensor [B,C] of 1-based answer ids (0 = empty entry),
-- C <= 32; the criterion head is normalised over a sample's candidates only (VQA v1: its 18 choices).  nil detaches
-- them.  slot as in setAnswers; the list lasts until the next batch goes into that slot.
function RAU:setCandidates(cand, slot)
  if cand == nil then
    check(C.rau_set_candidates(self.h, slot or -1, 0, nil))
    return
  end
  cand = cand:int():contiguous()
  assert(cand:dim() == 2 and cand:size(1) == self.n, 'cand must be [B,C]')
  check(C.rau_set_candidates(self.h, slot or -1, cand:size(2), cand:data()))
end
-- C of the resident batch's candidates, 0 without them
function RAU:batchCandidates()
  local c = ffi.new('int32_t[1]')
  check(C.rau_batch_candidates(self.h, c))
  return c[0]
end
-- MC statistics of the last forward on a batch with candidates (feval rule): loss (restricted criterion), correct,
-- score per row of nHop+2 (hops, uni, select) and the number of labelled rows
function RAU:candStats()
  local R = self.cfg.H + 2
  local loss, score = torch.FloatTensor(R), torch.FloatTensor(R)
  local correct = torch.IntTensor(R)
  local nlab = ffi.new('int32_t[1]')
  check(C.rau_cand_stats(self.h, loss:data(), correct:data(), score:data(), nlab))
  return {loss = loss, correct = correct, score = score, n_lab = nlab[0]}
end
-- the k best candidates of every predict_result row of the last forward: ids (IntTensor, 1-based, 0 behind the live
-- candidates), their logits and their confidences over the candidates, each [nHop+2, B, k]
function RAU:topkCand(k)
  local H, B = self.cfg.H, self.n
  local ids = torch.IntTensor(H + 2, B, k)
  local score, conf = torch.FloatTensor(H + 2, B, k), torch.FloatTensor(H + 2, B, k)
  check(C.rau_topk_cand(self.h, k, ids:data(), score:data(), conf:data()))
  return ids, score, conf
end
-- the per-sample loss rows [H][B] of the last forward (with weights: the weighted rows) as a FloatTensor
function RAU:lossRows()
  local t = torch.FloatTensor(self.cfg.H, self.n)
  check(C.rau_get_loss_rows(self.h, t:data()))
  return t
end

-- Attention targets (rau_set_att_targets): t FloatTensor [B,S] (or [B,W,H]), entries finite and >= 0, one target map
-- per SAMPLE; a row of zeros is an unsupervised sample.  backward(hop_w, select_w, att_w) then adds
-- att_w[h] * mean_b sum_s t (-log(attprob_h + 1e-12)) to the objective.  slot as in setAnswers; the targets last
-- until the next batch goes into that slot, and may be set after the forward.
function RAU:setAttTargets(t, slot)
  t = t:float():contiguous()
  assert(t:size(1) == self.n and t:nElement() == self.n * self.cfg.S, 't must be [B,S]')
  check(C.rau_set_att_targets(self.h, slot or -1, t:data()))
end
-- whether the resident batch carries attention targets
function RAU:batchAttTargets()
  local v = ffi.new('int[1]')
  check(C.rau_batch_att_targets(self.h, v))
  return v[0] ~= 0
end
-- ATT loss [H], attention mass on the target [H], pointing-game hits [H] (Lua tables) and the number of
-- supervised rows, of the last forward against its batch's targets
function RAU:attStats()
  local H = self.cfg.H
  local l, m = ffi.new('float[?]', H), ffi.new('float[?]', H)
  local hits, n = ffi.new('int32_t[?]', H), ffi.new('int32_t[1]')
  check(C.rau_att_stats(self.h, l, m, hits, n))
  local loss, mass, hit = {}, {}, {}
  for i = 1, H do loss[i] = l[i - 1]; mass[i] = m[i - 1]; hit[i] = hits[i - 1] end
  return loss, mass, hit, n[0]
end

-- A batch whose questions share feature maps: feats is the image TABLE [N,D,W,H] (Float- or HalfTensor, or a
-- ByteTensor of fp8 codes with feat_type 'e4m3' | 'e5m2'),
-- image_of an IntTensor [B] of 1-BASED table rows, as Torch indexes (feats:index(1, image_of:long()) is the
-- plain batch); converted here to the 0-based row offsets of rau_set_batch_images.  Only the N maps are
-- uploaded and, in evaluate mode, convolved.  slot = nil: the synchronous form.
function RAU:setBatchImages(feats, image_of, x, x_len, y, slot, has_labels, feat_type)
  follow_rows(self, x_len)
  local ft = feat_type_of(feats, feat_type)
  local idx = image_of:int():add(-1)
  if slot then
    check(C.rau_set_batch_async_images(self.h, slot, feats:data(), ft, feats:size(1), idx:data(), x:data(),
                                       x_len:data(), y and y:data() or nil, (has_labels == false) and 0 or 1))
  else
    check(C.rau_set_batch_images(self.h, feats:data(), ft, feats:size(1), idx:data(), x:data(), x_len:data(),
                                 y and y:data() or nil))
  end
end
-- Packed region features (rau_set_batch_packed): rows is a Float/HalfTensor [sum(counts), D] (or a ByteTensor of
-- fp8 codes with its feat_type), one row per box as the region files store them; counts an IntTensor [N] with
-- 1 <= counts[i] <= S, map i owning counts[i] consecutive rows.  Only the rows are uploaded; the device transposes
-- and zero-pads them and the counts become the batch's region counts (as by setRegions).  image_of nil: a plain
-- batch, N == B; else an IntTensor [B] of 1-BASED map numbers, as in setBatchImages (counts are then per image).
-- slot = nil: the synchronous form; slot = 0 | 1 with rows nil: the rows already lie at the start of the slot's staging.
function RAU:setBatchPacked(rows, counts, x, x_len, y, image_of, slot, has_labels, feat_type)
  follow_rows(self, x_len)
  local ft = feat_type_of(rows, feat_type)
  local n = counts:int():contiguous()
  assert(n:dim() == 1 and (image_of or n:size(1) == self.n), 'counts must be [B] (or [N] beside image_of)')
  assert(not rows or (rows:dim() == 2 and rows:size(1) == n:sum() and rows:size(2) == self.cfg.D),
         'rows must be [sum(counts), D]')
  local idx = image_of and image_of:int():add(-1)
  if slot then
    check(C.rau_set_batch_async_packed(self.h, slot, rows and rows:data() or nil, ft, n:size(1), n:data(),
                                       idx and idx:data() or nil, x and x:data() or nil,
                                       x_len and x_len:data() or nil, y and y:data() or nil,
                                       (has_labels == false) and 0 or 1))
  else
    check(C.rau_set_batch_packed(self.h, rows:data(), ft, n:size(1), n:data(), idx and idx:data() or nil, x:data(),
                                 x_len:data(), y and y:data() or nil))
  end
end
-- 0 for a plain resident batch, else the number of maps in its image table
-- Feature bank: every image's map once in device memory (rau_bank_*).  bankCreate(capacity, 'f32' | 'f16' |
-- 'bf16' | 'e4m3' | 'e5m2'); bankPut(first, feats) takes a Float/HalfTensor [n,D,W,H] (or a ByteTensor of fp8
-- codes with its feat_type) into the 1-based rows first .. first+n-1.  FloatTensors into a 16-bit or fp8 bank
-- are narrowed on the device: round to nearest even; fp8 saturates at the largest finite value (448 / 57344).
function RAU:bankCreate(capacity, feat_type)
  check(C.rau_bank_create(self.h, capacity, FEAT[feat_type or 'f32']))
end
function RAU:bankPut(first, feats, feat_type)
  local ft = feat_type_of(feats, feat_type)
  check(C.rau_bank_put(self.h, first - 1, feats:size(1), feats:data(), ft))
end
-- bankPut for packed region rows: rows [sum(counts), D], counts IntTensor [n]; the bank keeps the dense maps and
-- no counts (keep them on the host and pass setRegions what a bank batch needs).
function RAU:bankPutPacked(first, rows, counts, feat_type)
  local ft = feat_type_of(rows, feat_type)
  local n = counts:int():contiguous()
  assert(rows:dim() == 2 and rows:size(1) == n:sum() and rows:size(2) == self.cfg.D, 'rows must be [sum(counts), D]')
  check(C.rau_bank_put_packed(self.h, first - 1, n:size(1), rows:data(), ft, n:data()))
end
function RAU:bankDestroy()
  check(C.rau_bank_destroy(self.h))
end
-- setBatchImages with the table taken from the bank: rows [N] Int/LongTensor of 1-BASED bank rows, image_of [B]
-- 1-based positions in `rows`.  No feature map is read, staged or uploaded.  slot = nil: the synchronous form.
function RAU:setBatchBank(rows, image_of, x, x_len, y, slot, has_labels)
  follow_rows(self, x_len)
  local r = rows:int():add(-1)
  local idx = image_of:int():add(-1)
  if slot then
    check(C.rau_set_batch_async_bank(self.h, slot, r:size(1), r:data(), idx:data(), x:data(), x_len:data(),
                                     y and y:data() or nil, (has_labels == false) and 0 or 1))
  else
    check(C.rau_set_batch_bank(self.h, r:size(1), r:data(), idx:data(), x:data(), x_len:data(),
                               y and y:data() or nil))
  end
end

function RAU:batchImages()
  local n = ffi.new('int[1]')
  check(C.rau_batch_images(self.h, n))
  return n[0]
end

-- forward half of feval (SS:443-520); returns per-hop losses as a Lua table
function RAU:forward(seed, step)
  if seed then check(C.rau_set_dropout_seed(self.h, seed, step or 0)) end
  check(C.rau_forward(self.h))
  local H = self.cfg.H
  local l = ffi.new('float[?]', H)
  check(C.rau_get_losses(self.h, l))
  local t = {}
  for i = 1, H do t[i] = l[i - 1] end
  return t
end

-- backward half (SS:561-596); hop_w = per-hop criterion-gradient scale (SS:569 / Full:587-589)
-- select_w (optional) = per-hop weight of the step-selection head's BCE gradient: the multiplier the reference
-- fixes at 0 in d_do_pred:mul(0), SS:566; nil keeps that zero
-- att_w (optional) = per-hop weight of the attention supervision against setAttTargets' maps, where the reference
-- passes gradattprob = zeros (SS:361, 573); nil keeps those zeros
-- merge_w (optional) = {w_uni, w_sel}, the weights of the cross-entropies of the merged uni and select rows, which
-- the reference only logs (SS:521-557: stepStats' loss[H+1] and loss[H+2]); nil keeps them out of the objective
local function hop_array(H, t)
  local w = ffi.new('float[?]', H)
  for i = 1, H do w[i - 1] = t[i] end
  return w
end
local function merge_array(t)
  local w = ffi.new('float[2]')
  w[0], w[1] = t[1], t[2]
  return w
end
-- the weight arguments of the entry points: a term left out is nil (NULL), and the last one given picks the entry point
local function loss_args(H, hop_w, select_w, att_w, merge_w)
  return hop_array(H, hop_w), select_w and hop_array(H, select_w) or nil, att_w and hop_array(H, att_w) or nil,
         merge_w and merge_array(merge_w) or nil
end
function RAU:backward(hop_w, select_w, att_w, merge_w)
  local w, sw, aw, mw = loss_args(self.cfg.H, hop_w, select_w, att_w, merge_w)
  if mw then check(C.rau_backward_merged(self.h, w, sw, aw, mw))
  elseif aw then check(C.rau_backward_att(self.h, w, sw, aw))
  elseif sw then check(C.rau_backward_select(self.h, w, sw))
  else check(C.rau_backward(self.h, w)) end
end

-- the outputs of the last forward in device memory (rau_outputs_dev): logits [H,n,K] (rows at logitsPitch()), dopred [H,n] and attprob
-- [H,n,pitch] as const float* cdata plus the pitch; valid until the next forward, ordered on the ctx's stream
function RAU:outputsDev()
  local lg, dp, at = ffi.new('const float*[1]'), ffi.new('const float*[1]'), ffi.new('const float*[1]')
  local pitch = ffi.new('int32_t[1]')
  check(C.rau_outputs_dev(self.h, lg, dp, at, pitch))
  return lg[0], dp[0], at[0], pitch[0]
end

-- row pitch of outputsDev()'s logits (rau_logits_pitch): K where K % 4 == 0, else K rounded up to a multiple of 4
-- with +0 in columns K..pitch-1
function RAU:logitsPitch()
  local pitch = ffi.new('int32_t[1]')
  check(C.rau_logits_pitch(self.h, pitch))
  return pitch[0]
end

-- Feature-map gradient (rau_set_feat_grad): with the switch on every backward / graphStep also leaves the gradient
-- at the feature map behind, for a trainable stage in front of the library.  perImage false / nil
-- (RAU_FEAT_GRAD_SAMPLES): batches with one map per sample only, the backward of an image-table or bank batch then
-- errors.  perImage true (RAU_FEAT_GRAD_IMAGES): an image-table batch leaves the gradient at the TABLE, [N,D,pitch],
-- each image's samples summed in ascending order; every other batch as without it; bank batches stay refused.
RAU.FEAT_GRAD_OFF, RAU.FEAT_GRAD_SAMPLES, RAU.FEAT_GRAD_IMAGES = 0, 1, 2
function RAU:wantFeatureGrad(on, perImage)
  local mode = (on == nil or on) and (perImage and RAU.FEAT_GRAD_IMAGES or RAU.FEAT_GRAD_SAMPLES) or RAU.FEAT_GRAD_OFF
  check(C.rau_set_feat_grad(self.h, mode))
  return self
end
-- the map count of the last backward's result (rau_feat_grad_rows): n, or the table's N under perImage
function RAU:featureGradRows()
  local rows = ffi.new('int32_t[1]')
  check(C.rau_feat_grad_rows(self.h, rows))
  return rows[0]
end
-- the last backward's result in device memory: const float* cdata [rows,D,pitch] and the pitch (rau_feat_grad_dev);
-- valid until the next forward, ordered on the ctx's stream
function RAU:featureGrad()
  local p, pitch = ffi.new('const float*[1]'), ffi.new('int32_t[1]')
  check(C.rau_feat_grad_dev(self.h, p, pitch))
  return p[0], pitch[0]
end
-- Per-position L2 normalisation of the batch's maps (rau_set_feat_norm): with the switch on every forward / graphStep
-- first normalises each position's channel vector, x / max(||x||_2, eps) in float32 whatever the stored type, and runs
-- on the result as on a float32 batch; with wantFeatureGrad the gradient goes back through it to the raw maps.
-- on = false goes back to the maps as stored; eps defaults to 1e-12.  Between steps; a change drops the last forward.
RAU.XNORM_NONE, RAU.XNORM_L2 = 0, 1
function RAU:normalizeFeatures(on, eps)
  check(C.rau_set_feat_norm(self.h, (on == nil or on) and RAU.XNORM_L2 or RAU.XNORM_NONE, eps or 1e-12))
  return self
end
-- kind (RAU.XNORM_*) and eps (rau_feat_norm)
function RAU:featNorm()
  local kind, eps = ffi.new('int[1]'), ffi.new('float[1]')
  check(C.rau_feat_norm(self.h, kind, eps))
  return kind[0], eps[0]
end
-- the last forward's normalised maps in device memory: const float* cdata xn [rows,D,pitch] and nrm [rows,pitch], the
-- pitch and the map count (rau_norm_feats_dev: N after the evaluate-mode forward of an image table, else n); valid
-- until the next forward, ordered on the ctx's stream
function RAU:normFeats()
  local xn, nrm = ffi.new('const float*[1]'), ffi.new('const float*[1]')
  local pitch, rows = ffi.new('int32_t[1]'), ffi.new('int32_t[1]')
  check(C.rau_norm_feats_dev(self.h, xn, nrm, pitch, rows))
  return xn[0], nrm[0], pitch[0], rows[0]
end
-- setBatch with the maps already on the device: feats_dev a DEVICE float* to dense [n,D,S] float32, ordered by the
-- caller in front of the ctx's stream (rau_set_batch_dev); x, x_len, y host tensors as in setBatch
function RAU:setBatchDev(feats_dev, x, x_len, y)
  follow_rows(self, x_len)
  check(C.rau_set_batch_dev(self.h, feats_dev, x:data(), x_len:data(), y and y:data() or nil))
end
-- Question state from the caller (rau_set_question_dev): q a DEVICE pointer to dense [n,Q] (Q = 4 Rq) elements of
-- qtype 'f32' (default), 'f16' or 'bf16', ordered by the caller in front of the ctx's stream.  It attaches to the
-- resident batch: forward / graphStep then read it in place of the built-in encoder's output and launch nothing of
-- the encoder, the backward leaves questionGrad() behind and does not touch the embed and rnn gradients.  q == nil
-- detaches it, and so does the next setBatch* / useBatch / setBatchSize.
RAU.QUESTION_TYPES = {f32 = 0, f16 = 1, bf16 = 2}
function RAU:setQuestionDev(q, qtype)
  local t = RAU.QUESTION_TYPES[qtype or 'f32']
  assert(t, 'setQuestionDev: qtype is one of f32, f16, bf16')
  check(C.rau_set_question_dev(self.h, q, t))
  return self
end
function RAU:batchQuestion()
  local has = ffi.new('int[1]')
  check(C.rau_batch_question(self.h, has))
  return has[0] ~= 0
end
-- the last backward's gradient at the attached question in device memory: const float* cdata [n,Q]
-- (rau_question_grad_dev); valid until the next forward, ordered on the ctx's stream
function RAU:questionGrad()
  local p = ffi.new('const float*[1]')
  check(C.rau_question_grad_dev(self.h, p))
  return p[0]
end
-- setBatchImages with the table already on the device: table_dev a DEVICE float* to dense [n_images,D,S] float32,
-- image_of an IntTensor [B] of 1-BASED table rows (rau_set_batch_dev_images)
function RAU:setBatchDevImages(table_dev, n_images, image_of, x, x_len, y)
  follow_rows(self, x_len)
  local idx = image_of:int():add(-1)
  check(C.rau_set_batch_dev_images(self.h, table_dev, n_images, idx:data(), x:data(), x_len:data(),
                                   y and y:data() or nil))
end

-- backward with the gradients of a term of the caller's own at those outputs (rau_backward_ext): grads = { logits =,
-- dopred =, attprob = }, each a DEVICE float* (dense [H,n,K], [H,n], [H,n,S]) or nil; hop_w may be nil (zeros) then,
-- and the batch needs labels only for a non-zero hop_w, select_w or merge_w
function RAU:backwardExt(hop_w, select_w, att_w, merge_w, grads)
  local H = self.cfg.H
  local w = hop_w and hop_array(H, hop_w) or nil
  local sw = select_w and hop_array(H, select_w) or nil
  local aw = att_w and hop_array(H, att_w) or nil
  local mw = merge_w and merge_array(merge_w) or nil
  local g = nil
  if grads then
    g = ffi.new('rau_out_grads')
    g.d_logits, g.d_dopred, g.d_attprob = grads.logits, grads.dopred, grads.attprob
  end
  check(C.rau_backward_ext(self.h, w, sw, aw, mw, g))
end

-- Initial state of the hop chain from the caller (rau_set_state_dev): c0, h0 DEVICE pointers to dense [n,R] elements
-- of stype 'f32' (default), 'f16' or 'bf16', ordered by the caller in front of the ctx's stream.  It attaches to the
-- resident batch: forward / graphStep start hop 0 from it, every backward leaves stateGrad() behind.  Both nil
-- detach it, and so does the next setBatch* / useBatch / setBatchSize.  The copy is taken at the call, so c0, h0 may
-- be the last hop's rows of stateDev(): carrying the state is one call.
function RAU:setStateDev(c0, h0, stype)
  local t = RAU.QUESTION_TYPES[stype or 'f32']
  assert(t, 'setStateDev: stype is one of f32, f16, bf16')
  check(C.rau_set_state_dev(self.h, c0, h0, t))
  return self
end
function RAU:batchState()
  local has = ffi.new('int[1]')
  check(C.rau_batch_state(self.h, has))
  return has[0] ~= 0
end
-- c' and h' of every hop of the last step-level forward in device memory: two const float* cdata [H,n,R]
-- (rau_state_dev); valid until the next forward, ordered on the ctx's stream
function RAU:stateDev()
  local c, h = ffi.new('const float*[1]'), ffi.new('const float*[1]')
  check(C.rau_state_dev(self.h, c, h))
  return c[0], h[0]
end
-- backwardExt with the gradients of the caller's term at the hop states as well (rau_backward_state): sgrads =
-- { h =, c_last = }, DEVICE float* to dense [H,n,R] (every hop's h') and [n,R] (the last hop's c'), or nil
function RAU:backwardState(hop_w, select_w, att_w, merge_w, grads, sgrads)
  local H = self.cfg.H
  local w = hop_w and hop_array(H, hop_w) or nil
  local sw = select_w and hop_array(H, select_w) or nil
  local aw = att_w and hop_array(H, att_w) or nil
  local mw = merge_w and merge_array(merge_w) or nil
  local g, sg = nil, nil
  if grads then
    g = ffi.new('rau_out_grads')
    g.d_logits, g.d_dopred, g.d_attprob = grads.logits, grads.dopred, grads.attprob
  end
  if sgrads then
    sg = ffi.new('rau_state_grads')
    sg.d_h, sg.d_c_last = sgrads.h, sgrads.c_last
  end
  check(C.rau_backward_state(self.h, w, sw, aw, mw, g, sg))
end
-- the last backward's gradient at the attached initial state in device memory: d_c0, d_h0, const float* cdata [n,R]
-- (rau_state_grad_dev); valid until the next forward, ordered on the ctx's stream
function RAU:stateGrad()
  local dc, dh = ffi.new('const float*[1]'), ffi.new('const float*[1]')
  check(C.rau_state_grad_dev(self.h, dc, dh))
  return dc[0], dh[0]
end

-- Additive attention bias from the caller (rau_set_att_bias_dev): b a DEVICE pointer to dense [n,S] elements of btype
-- 'f32' (default), 'f16' or 'bf16', ordered by the caller in front of the ctx's stream; -inf = no attention there.  It
-- attaches to the resident batch: every hop of forward / graphStep adds it to the attention scores, every backward
-- leaves attBiasGrad() behind.  nil detaches it, and so does the next setBatch* / useBatch / setBatchSize.
function RAU:setAttBiasDev(b, btype)
  local t = RAU.QUESTION_TYPES[btype or 'f32']
  assert(t, 'setAttBiasDev: btype is one of f32, f16, bf16')
  check(C.rau_set_att_bias_dev(self.h, b, t))
  return self
end
function RAU:batchAttBias()
  local has = ffi.new('int[1]')
  check(C.rau_batch_att_bias(self.h, has))
  return has[0] ~= 0
end
-- the last backward's gradient at the attached bias in device memory: const float* cdata [n,pitch] and the row pitch
-- in floats (rau_att_bias_grad_dev); valid until the next forward, ordered on the ctx's stream
function RAU:attBiasGrad()
  local d, pitch = ffi.new('const float*[1]'), ffi.new('int32_t[1]')
  check(C.rau_att_bias_grad_dev(self.h, d, pitch))
  return d[0], tonumber(pitch[0])
end

-- zeroGradParameters (unless zero_grads == false) + forward + backward as one captured graph launch
function RAU:graphStep(hop_w, select_w, zero_grads, att_w, merge_w)
  local w, sw, aw, mw = loss_args(self.cfg.H, hop_w, select_w, att_w, merge_w)
  local z = (zero_grads == false) and 0 or 1
  if mw then check(C.rau_graph_step_merged(self.h, w, sw, aw, mw, z))
  elseif aw then check(C.rau_graph_step_att(self.h, w, sw, aw, z))
  else check(C.rau_graph_step_select(self.h, w, sw, z)) end
end

function RAU:zeroGradParameters() check(C.rau_zero_grads(self.h)) end

-- noise + clip + adam x 3 groups (SS:597-630, 770-772)
function RAU:update(step_t, lr, mult_lr, eta, gamma, clip, seed)
  local norms = ffi.new('float[3]')
  check(C.rau_noise_clip_adam(self.h, step_t, lr, mult_lr, 0.9, 0.999, 1e-8, eta or 0.01,
                              gamma or 0.55, clip or 0.1, seed or 0, norms))
  return norms[0], norms[1], norms[2]
end

-- the same step with a rule and a clip scope (rau_update): opts = { rule = 'adam' | 'adamax', clip_scope =
-- 'group' | 'global', step_t =, lr =, mult_lr =, beta1 =, beta2 =, eps =, eta =, gamma =, clip =, seed = }; what
-- is left out keeps rau_update_opts_default's value.  'adam' with 'group' is rau:update, bit for bit; 'adamax' and
-- 'global' are not in the reference.  Returns the three group norms and the global norm.
local RULE = { adam = 0, adamax = 1 }
local SCOPE = { group = 0, global = 1 }
function RAU:updateWith(opts)
  local o = ffi.new('rau_update_opts[1]')
  C.rau_update_opts_default(o)
  if opts.rule then o[0].rule = assert(RULE[opts.rule], 'updateWith: unknown rule') end
  if opts.clip_scope then o[0].clip_scope = assert(SCOPE[opts.clip_scope], 'updateWith: unknown clip_scope') end
  for _, k in ipairs({ 'lr', 'mult_lr', 'beta1', 'beta2', 'eps', 'eta', 'gamma', 'clip' }) do
    if opts[k] then o[0][k] = opts[k] end
  end
  if opts.seed then o[0].noise_seed = opts.seed end
  local norms = ffi.new('float[4]')
  check(C.rau_update(self.h, opts.step_t or 0, o, norms))
  return norms[0], norms[1], norms[2], norms[3]
end

-- rau:updateWith's step with decoupled weight decay, per-layer options and the weight average (rau_update_ex): the
-- fields of rau:updateWith plus weight_decay = (AdamW's order, under 'adamax' too) and ema_decay = (needs
-- rau:emaReset() first).  Frozen layers are in none of the four norms returned.
function RAU:updateEx(opts)
  local o = ffi.new('rau_update_opts[1]')
  C.rau_update_opts_default(o)
  if opts.rule then o[0].rule = assert(RULE[opts.rule], 'updateEx: unknown rule') end
  if opts.clip_scope then o[0].clip_scope = assert(SCOPE[opts.clip_scope], 'updateEx: unknown clip_scope') end
  for _, k in ipairs({ 'lr', 'mult_lr', 'beta1', 'beta2', 'eps', 'eta', 'gamma', 'clip' }) do
    if opts[k] then o[0][k] = opts[k] end
  end
  if opts.seed then o[0].noise_seed = opts.seed end
  local x = ffi.new('rau_update_extras[1]')
  C.rau_update_extras_default(x)
  if opts.weight_decay then x[0].weight_decay = opts.weight_decay end
  if opts.ema_decay then x[0].ema_decay = opts.ema_decay end
  local norms = ffi.new('float[4]')
  check(C.rau_update_ex(self.h, opts.step_t or 0, o, x, norms))
  return norms[0], norms[1], norms[2], norms[3]
end
-- one layer's options: group 'embed' | 'rnn' | 'mult', index = the layer's 0-based place in its group (its weight
-- and bias are entries 2 index and 2 index + 1 of the layout); nil keeps the value.  lr_scale = 0 freezes the layer.
function RAU:setLayerOpts(group, index, lr_scale, decay_weight, decay_bias)
  local v = ffi.new('float[3]')
  check(C.rau_get_layer_opts(self.h, GROUP[group], index, v, v + 1, v + 2))
  check(C.rau_set_layer_opts(self.h, GROUP[group], index, lr_scale or v[0], decay_weight or v[1],
                             decay_bias or v[2]))
end
-- the weight average: emaReset() starts it at the current weights; emaSwap() exchanges weights and average in
-- place (evaluate, then swap back: every update is refused while swapped) and returns the new `swapped` flag
function RAU:emaReset() check(C.rau_ema_reset(self.h)) end
function RAU:emaSwap()
  check(C.rau_ema_swap(self.h))
  local sw = ffi.new('int[1]')
  check(C.rau_ema_state(self.h, nil, sw))
  return sw[0] == 1
end

-- per-layer statistics, computed on the device (rau_layer_stats): what = a sum of 1 (gradients), 2 (weights) and
-- 4 (the rule's direction m / (sqrt(v) + eps) or adamax's m / u; needs an update to have run), eps = the rule's.
-- Returns a 1-based table with one record per layout entry, embed then rnn then mult: { n =, sumsq = {g, p, d},
-- absmax = {g, p, d}, nonfinite = {g, p, d} } over the FINITE elements; what was not asked for is 0.  Synchronises.
function RAU:layerStats(what, eps)
  local n = C.rau_layer_stats_count(self.h)
  local rec = ffi.new('rau_layer_stat[?]', n)
  check(C.rau_layer_stats(self.h, what or 1, eps or 1e-8, rec))
  local out = {}
  for i = 1, n do
    local r = rec[i - 1]
    out[i] = { n = tonumber(r.n), sumsq = { r.sumsq[0], r.sumsq[1], r.sumsq[2] },
               absmax = { r.absmax[0], r.absmax[1], r.absmax[2] },
               nonfinite = { tonumber(r.nonfinite[0]), tonumber(r.nonfinite[1]), tonumber(r.nonfinite[2]) } }
  end
  return out
end
-- the non-finite guard: mode 1 makes rau:update / updateWith / updateEx count the non-finite gradient elements first
-- (one more read of the gradients and a stream synchronisation) and SKIP a poisoned step -- nothing changes, the
-- norms come back NaN; mode 0 (the default) switches it off.  A NaN in accumulated gradients stays until
-- rau:zeroGradParameters().
function RAU:setUpdateGuard(mode) check(C.rau_set_update_guard(self.h, mode or 1)) end
-- -> mode, updates skipped so far, whether the last update was skipped, and the non-finite counts that last skipped
-- update found per group { embed, rnn, mult }
function RAU:updateGuard()
  local mode, skipped, last = ffi.new('int[1]'), ffi.new('int64_t[1]'), ffi.new('int32_t[1]')
  local nf = ffi.new('int64_t[3]')
  check(C.rau_update_guard(self.h, mode, skipped, last, nf))
  return mode[0], tonumber(skipped[0]), last[0] == 1, { tonumber(nf[0]), tonumber(nf[1]), tonumber(nf[2]) }
end

-- optimizer state of one group: m, v (FloatTensors of the group's length, filled; v holds the u of adamax),
-- then t and the rule name.  Before the first update: zeros, 0, 'adam'.
function RAU:optState(group, m, v)
  local t, r = ffi.new('int64_t[1]'), ffi.new('int32_t[1]')
  check(C.rau_get_opt_state(self.h, GROUP[group], m and m:data() or nil, v and v:data() or nil, t, r))
  return tonumber(t[0]), (r[0] == 1) and 'adamax' or 'adam'
end
-- rau:setOptState(group, m, v, t, rule); m = v = nil with t = 0 resets the group to `rule`
function RAU:setOptState(group, m, v, t, rule)
  check(C.rau_set_opt_state(self.h, GROUP[group], m and m:data() or nil, v and v:data() or nil, t or 0,
                            assert(RULE[rule or 'adam'], 'setOptState: unknown rule')))
end

-- answers: IntTensor [H,B] of 1-based class ids (torch.max first-max rule, SS:488)
function RAU:answers(out) check(C.rau_get_argmax(self.h, out:data())); return out end
function RAU:logits(out) check(C.rau_get_logits(self.h, out:data())); return out end
function RAU:attention(out) check(C.rau_get_attention(self.h, out:data())); return out end
function RAU:sync() check(C.rau_sync(self.h)) end

-- feval's bookkeeping of the last forward (SS:476-556), on the device: tab_loss (nHop+2: per-hop CE,
-- uni CE, select CE), tab_loss_do_pred (nHop: BCE of do_pred vs argmax_h == y) and the counts the
-- accuracy tables add up (SS:491, 526, 536, 552-553), all 1-based Lua tables.  Valid from the
-- forward through its backward.
function RAU:stepStats()
  local H = self.cfg.H
  local l, d, c = ffi.new('float[?]', H + 2), ffi.new('float[?]', H), ffi.new('int32_t[?]', 4 * H + 3)
  check(C.rau_step_stats(self.h, l, d, c))
  local tab_loss, tab_loss_do_pred = {}, {}
  local counts = { correct = {}, do_pred_correct = {}, fired = {}, selected = {}, did_correct = c[2 * H + 2] }
  for i = 1, H + 2 do tab_loss[i] = l[i - 1]; counts.correct[i] = c[i - 1] end
  for h = 1, H do
    tab_loss_do_pred[h] = d[h - 1]
    counts.do_pred_correct[h] = c[H + 2 + h - 1]
    counts.fired[h] = c[2 * H + 3 + h - 1]
    counts.selected[h] = c[3 * H + 3 + h - 1]
  end
  return tab_loss, tab_loss_do_pred, counts
end

-- Metric scores of the last forward's answers against its batch's answer set (feval rule, as stepStats):
-- FloatTensor [nHop+2, B] (hops, uni, select) and their batch sums as a 1-based Lua table.  With score =
-- min(#humans / 3, 1) the sums are the VQA accuracy times B.
function RAU:stepScores()
  local H, B = self.cfg.H, self.n
  local per, tot = torch.FloatTensor(H + 2, B), ffi.new('float[?]', H + 2)
  check(C.rau_step_scores(self.h, per:data(), tot))
  local t = {}
  for i = 1, H + 2 do t[i] = tot[i - 1] end
  return per, t
end
-- The same for the answers of the last predict() (last hop forced): oe scores, mc scores (nil without an MC
-- list), and their batch sums { oe = {..}, mc = {..} | nil }
function RAU:predictScores(with_mc)
  local H, B = self.cfg.H, self.n
  local oe, mc = torch.FloatTensor(H + 2, B), with_mc and torch.FloatTensor(H + 2, B) or nil
  local tot = ffi.new('float[?]', 2 * (H + 2))
  check(C.rau_predict_scores(self.h, oe:data(), mc and mc:data() or nil, tot))
  local t = { oe = {}, mc = with_mc and {} or nil }
  for i = 1, H + 2 do
    t.oe[i] = tot[i - 1]
    if with_mc then t.mc[i] = tot[H + 2 + i - 1] end
  end
  return oe, mc, t
end

-- predict_result + the eval loop's answer selection (SS:633-705, 877-900) on the last forward
-- (evaluate mode): returns oe, mc as IntTensors [nHop+2, B] of 1-based answer ids (hops, uni,
-- select); ans_mc: IntTensor [B, nMultChoice] (0 = empty slot) or nil (mc = nil)
function RAU:predict(ans_mc)
  local H, B = self.cfg.H, self.n
  local oe = torch.IntTensor(H + 2, B)
  if not ans_mc then
    check(C.rau_predict(self.h, nil, 0, oe:data(), nil))
    return oe, nil
  end
  ans_mc = ans_mc:int():contiguous()
  local mc = torch.IntTensor(H + 2, B)
  check(C.rau_predict(self.h, ans_mc:data(), ans_mc:size(2), oe:data(), mc:data()))
  return oe, mc
end

-- the k best open-ended answers of every predict_result row (hops, uni, select; last hop forced) of
-- the last forward: ids (IntTensor, 1-based, ids[{r, b, 1}] == predict()'s oe[{r, b}]), their logits and
-- their softmax confidences (FloatTensors), each [nHop+2, B, k], best first, ties by the lower id
function RAU:topk(k)
  local H, B = self.cfg.H, self.n
  local ids = torch.IntTensor(H + 2, B, k)
  local score, conf = torch.FloatTensor(H + 2, B, k), torch.FloatTensor(H + 2, B, k)
  check(C.rau_topk(self.h, k, ids:data(), score:data(), conf:data()))
  return ids, score, conf
end

-- data parallel (one process per GPU): rank 0 calls RAU.commId() and ships the 128-byte string
-- to the other ranks (file, socket, ...); every rank then calls rau:commInit(n, rank, id) once
-- and rau:allreduceGrads() between rau:backward(w) and rau:update(...)
function RAU.commId()
  local id = ffi.new('char[128]')
  check(C.rau_comm_unique_id(id, 128))
  return ffi.string(id, 128)
end
function RAU:commInit(nranks, rank, id) check(C.rau_comm_init(self.h, nranks, rank, id, #id)) end
function RAU:allreduceGrads() check(C.rau_allreduce_grads(self.h)) end

-- Device tensors ---------------------------------------------------------------
-- What feval's loops do BETWEEN module calls (`rnn_out[k] = lst[k]`, `uni_pred:add(pred[1])`,
-- `torch.max(pred[1], 2)`, `ans:eq(y):sum()`, SS:455-461, 482-492, 522-526, 584-591) needs
-- tensor-shaped values.  cutorch does not exist on an MI355X host, so the clones below return
-- RAU.Tensor objects: {ptr = device float*, size = {rows, cols}, rau = owner}, dense row-major,
-- with the handful of methods those loops use, each one small C-ABI call (rau_dev_*).
-- Views of ctx-owned slots keep nn.Module's self.output lifetime; RAU.Tensor.new allocates.
local Tensor = {}
local IntTensor = {}
local function numel(sz) local n = 1; for _, v in ipairs(sz) do n = n * v end; return n end
-- Owned device memory is returned to the context when its tensor is collected (or by :free());
-- the finalizer sits on the pointer cdata, so views (which copy the address, not the cdata) never
-- free anything.
local function dev_alloc(rau, n)
  local p = ffi.new('float*[1]')
  check(C.rau_dev_alloc(rau.h, n, p))
  local h, life = rau.h, rau.life
  return ffi.gc(p[0], function(q) if life.alive then C.rau_dev_free(h, q) end end)
end
local function dev_release(t)
  if t.owned then
    local q = ffi.gc(t.ptr, nil)
    t.owned = false
    if t.rau.life.alive then check(C.rau_dev_free(t.rau.h, ffi.cast('float*', q))) end
  end
end
local function ptr_of(x) if type(x) == 'table' then return x.ptr end; return x end

Tensor.__index = function(t, k)
  if type(k) == 'number' then return Tensor.row(t, k) end     -- t[k]: 1-based row view
  return Tensor[k]
end
Tensor.__newindex = function(t, k, v)
  if type(k) == 'number' then Tensor.row(t, k):copy(v) else rawset(t, k, v) end   -- t[k] = row
end
function Tensor.wrap(rau, ptr, ...)
  return setmetatable({ rau = rau, ptr = ptr, size = { ... } }, Tensor)
end
function Tensor.new(rau, ...)                                  -- zero-filled, like torch.zeros
  local sz = { ... }
  return setmetatable({ rau = rau, ptr = dev_alloc(rau, numel(sz)), size = sz, owned = true }, Tensor)
end
function Tensor:nElement() return numel(self.size) end
function Tensor:dim() return #self.size end
function Tensor:row(k)                                         -- 1-based, view
  local cols = numel(self.size) / self.size[1]
  assert(k >= 1 and k <= self.size[1], 'row index out of range')
  local v = Tensor.wrap(self.rau, self.ptr + (k - 1) * cols, cols)
  -- pointer arithmetic on the cdata makes a NEW cdata without the finalizer: the view keeps a
  -- reference to its owner so that the owner (and the memory) outlives it
  rawset(v, 'base', rawget(self, 'base') or self)
  return v
end
function Tensor:zero() check(C.rau_dev_fill(self.rau.h, self.ptr, self:nElement(), 0)); return self end
function Tensor:fill(v) check(C.rau_dev_fill(self.rau.h, self.ptr, self:nElement(), v)); return self end
function Tensor:copy(src)                                      -- device tensor or host FloatTensor
  if getmetatable(src) == Tensor then
    assert(src:nElement() == self:nElement(), 'size mismatch')
    check(C.rau_dev_copy(self.rau.h, self.ptr, src.ptr, self:nElement()))
  else
    check(C.rau_dev_upload(self.rau.h, self.ptr, src:data(), self:nElement() * 4))
  end
  return self
end
function Tensor:clone() return Tensor.new(self.rau, unpack(self.size)):copy(self) end
function Tensor:add(a, x)                                      -- :add(x), :add(alpha, x) or :add(scalar)
  if x == nil and type(a) == 'number' then
    check(C.rau_dev_add_scalar(self.rau.h, self.ptr, self:nElement(), a)); return self
  end
  if x == nil then a, x = 1, a end
  assert(x:nElement() == self:nElement(), 'size mismatch')
  check(C.rau_dev_axpy(self.rau.h, self.ptr, x.ptr, self:nElement(), a)); return self
end
function Tensor:mul(a) check(C.rau_dev_scale(self.rau.h, self.ptr, self:nElement(), a)); return self end
-- what utils/optim_updates.lua's adam() does to its flat vectors (lines 76-86)
function Tensor:addcmul(a, x1, x2)                             -- self += a * x1 * x2
  check(C.rau_dev_addcmul(self.rau.h, self.ptr, a, x1.ptr, x2.ptr, self:nElement())); return self
end
function Tensor:addcdiv(a, x1, x2)                             -- self += a * x1 / x2
  check(C.rau_dev_addcdiv(self.rau.h, self.ptr, a, x1.ptr, x2.ptr, self:nElement())); return self
end
function Tensor:sqrt() check(C.rau_dev_sqrt(self.rau.h, self.ptr, self:nElement())); return self end
function Tensor:div(a) return self:mul(1 / a) end
function Tensor:sum()
  local o = ffi.new('double[1]')
  check(C.rau_dev_sum(self.rau.h, self.ptr, self:nElement(), o)); return o[0]
end
function Tensor:mean() return self:sum() / self:nElement() end
-- torch.max(t, 2): values [rows,1] and 1-based first-max indices [rows,1] (SS:488)
function Tensor:max(dim)
  assert(dim == 2 and #self.size == 2, 'only max over dimension 2 of a matrix')
  local r, c = self.size[1], self.size[2]
  -- results live in a ring of four context-owned slots per row count (feval calls this once per
  -- hop per iteration, SS:488: no allocation on that path); like self.output they stay valid
  -- until the slot comes round again
  local ring = self.rau.scratch[r]
  if not ring then
    ring = { k = 0 }
    for s = 1, 4 do ring[s] = { Tensor.new(self.rau, r, 1), IntTensor.new(self.rau, r, 1) } end
    self.rau.scratch[r] = ring
  end
  ring.k = ring.k % 4 + 1
  local v, i = ring[ring.k][1], ring[ring.k][2]
  check(C.rau_dev_rowmax(self.rau.h, self.ptr, r, c, v.ptr, i.ptr))
  return v, i
end
-- torch.topk(t, k, 2, true, true): values [rows,k], best first, and their 1-based indices [rows,k];
-- ties by the lower index, NaN last.  The results are the caller's (owned tensors).
function Tensor:topk(k)
  assert(#self.size == 2, 'only topk over dimension 2 of a matrix')
  local r, c = self.size[1], self.size[2]
  local v, i = Tensor.new(self.rau, r, k), IntTensor.new(self.rau, r, k)
  check(C.rau_dev_topk(self.rau.h, self.ptr, r, c, k, v.ptr, i.ptr))
  return v, i
end
-- dst rows k with key[k] == value take src's rows: the whole `for k=1,B do if x_len[k]==t ...`
-- loop of SS:455-461 / SS:584-591 as one call (key: device IntTensor)
function Tensor:selectRows(src, key, value)
  local r = self.size[1]
  check(C.rau_dev_select_rows(self.rau.h, self.ptr, src.ptr, r, self:nElement() / r, key.ptr, value))
  return self
end
function Tensor:float()                                        -- host copy (torch.FloatTensor)
  local t = torch.FloatTensor(unpack(self.size))
  check(C.rau_dev_download(self.rau.h, t:data(), self.ptr, self:nElement() * 4)); return t
end
function Tensor:free() dev_release(self) end

IntTensor.__index = IntTensor
function IntTensor.new(rau, ...)
  local sz = { ... }
  local base = dev_alloc(rau, numel(sz))                       -- 4-byte elements either way
  -- `base` carries the finalizer; the int32 view of it is what the calls take
  return setmetatable({ rau = rau, base = base, ptr = ffi.cast('int32_t*', base), size = sz,
                        owned = true }, IntTensor)
end
function IntTensor:free()
  if self.owned then
    local t = { rau = self.rau, ptr = self.base, owned = true }
    self.owned = false
    dev_release(t)
  end
end
function IntTensor:copy(src)                                   -- host IntTensor -> device
  check(C.rau_dev_upload(self.rau.h, self.ptr, src:data(), numel(self.size) * 4)); return self
end
function IntTensor:int()
  local t = torch.IntTensor(unpack(self.size))
  check(C.rau_dev_download(self.rau.h, t:data(), self.ptr, numel(self.size) * 4)); return t
end
-- ans:eq(y):sum() in one call (SS:489-492)
function IntTensor:eqSum(other)
  local o = ffi.new('int32_t[1]')
  check(C.rau_dev_count_eq(self.rau.h, self.ptr, other.ptr, numel(self.size), o)); return o[0]
end
RAU.Tensor, RAU.IntTensor = Tensor, IntTensor
function RAU:zeros(...) return Tensor.new(self, ...) end       -- torch.zeros(...):cuda()
function RAU:ints(host) return IntTensor.new(self, host:nElement()):copy(host) end

-- nn.Module surface completeness: parameters live on the device from the start and the clones
-- share them by construction, so these are identities (SS:319, 340-346); updateParameters is
-- never called by the reference (updates go through adam on the flat vectors, SS:770-772); for
-- hosts that do call it, it is nn.Module's plain SGD step x = x - lr * dx on all three groups.
function RAU:cuda() return self end
function RAU:clone() return self end
function RAU:float() return self end
function RAU:updateParameters(lr)
  for _, g in ipairs({ 'embed', 'rnn', 'mult' }) do
    local p = self:getParameters(g)
    check(C.rau_dev_axpy(self.h, p.ptr, p.grad, p.n, -lr))
  end
end
-- flat parameter / gradient vectors as device tensors: params, grads = rau:flat('mult')
function RAU:flat(group)
  local p = self:getParameters(group)
  return Tensor.wrap(self, p.ptr, p.n), Tensor.wrap(self, p.grad, p.n)
end

-- adam(x, dx, lr, beta1, beta2, epsilon, state): the signature and state fields of
-- utils/optim_updates.lua:59-87, for x, dx = rau:flat(group) -- so SS:770-772 runs unchanged.
-- state.m / state.v are device tensors created on first use (x.new(#dx):zero() in the reference),
-- state.t counts calls; the five tensor statements run as one pass (rau_dev_adam).  No state.tmp:
-- sqrt(v) + epsilon never leaves registers.
function RAU.adam(x, dx, lr, beta1, beta2, epsilon, state)
  beta1, beta2, epsilon = beta1 or 0.9, beta2 or 0.999, epsilon or 1e-8
  if not state.m then
    state.t = 0
    state.m = Tensor.new(x.rau, x:nElement())
    state.v = Tensor.new(x.rau, x:nElement())
  end
  state.t = state.t + 1
  check(C.rau_dev_adam(x.rau.h, x.ptr, dx.ptr, state.m.ptr, state.v.ptr, x:nElement(), lr, beta1, beta2,
                       epsilon, state.t))
end
-- its twin for adamax (not in the reference; the element arithmetic of rau:updateWith{rule = 'adamax'}):
-- state.m / state.u / state.t, kept as RAU.adam keeps its own
function RAU.adamax(x, dx, lr, beta1, beta2, epsilon, state)
  beta1, beta2, epsilon = beta1 or 0.9, beta2 or 0.999, epsilon or 1e-8
  if not state.m then
    state.t = 0
    state.m = Tensor.new(x.rau, x:nElement())
    state.u = Tensor.new(x.rau, x:nElement())
  end
  state.t = state.t + 1
  check(C.rau_dev_adamax(x.rau.h, x.ptr, dx.ptr, state.m.ptr, state.u.ptr, x:nElement(), lr, beta1, beta2,
                         epsilon, state.t))
end

-- Module-level clones ---------------------------------------------------------
-- For scripts that keep feval's own loops (SS:443-596).  Arguments are RAU.Tensor / RAU.IntTensor
-- objects (or raw device cdata pointers); results are RAU.Tensor VIEWS of ctx-owned slots that stay
-- valid until the same clone runs again (the lifetime of nn.Module's self.output).
-- Indices are 1-based like embed_clones[t] / lstm_clones[t] / multimodal_clones[h].
local function clone(self, kind, i)
  local m = { rau = self, i = i - 1 }
  local cfg, Q = self.cfg, 4 * self.cfg.Rq
  if kind == 'embed' then
    function m:forward(x_t)
      local o = ffi.new('float*[1]')
      check(C.rau_embed_forward(self.rau.h, self.i, ptr_of(x_t), o))
      self.output = Tensor.wrap(self.rau, o[0], self.rau.n, cfg.E)
      return self.output
    end
    function m:backward(x_t, d_we) check(C.rau_embed_backward(self.rau.h, self.i, ptr_of(x_t), ptr_of(d_we))) end
  elseif kind == 'rnn' then
    function m:forward(inp)   -- {x, state}
      local o = ffi.new('float*[1]')
      check(C.rau_deeplstm_forward(self.rau.h, self.i, ptr_of(inp[1]), ptr_of(inp[2]), o))
      self.output = Tensor.wrap(self.rau, o[0], self.rau.n, Q)
      return self.output
    end
    function m:backward(inp, d_state_out)
      local dx, ds = ffi.new('float*[1]'), ffi.new('float*[1]')
      check(C.rau_deeplstm_backward(self.rau.h, self.i, ptr_of(inp[1]), ptr_of(inp[2]),
                                    ptr_of(d_state_out), dx, ds))
      self.gradInput = { Tensor.wrap(self.rau, dx[0], self.rau.n, cfg.E), Tensor.wrap(self.rau, ds[0], self.rau.n, Q) }
      return self.gradInput
    end
  elseif kind == 'multimodal' then
    function m:forward(inp, regions)   -- {q, X, c, h}; regions: RAU.IntTensor [B] of region counts in device memory, or nil
      local o = {}
      for k = 1, 5 do o[k] = ffi.new('float*[1]') end
      check(C.rau_multimodal_forward_regions(self.rau.h, self.i, ptr_of(inp[1]), ptr_of(inp[2]),
                                             ptr_of(inp[3]), ptr_of(inp[4]), regions and ptr_of(regions) or nil,
                                             o[1], o[2], o[3], o[4], o[5]))
      local r = self.rau                                             -- {logits, dp, a, c, h}
      self.output = { Tensor.wrap(r, o[1][0], self.rau.n, cfg.K), Tensor.wrap(r, o[2][0], self.rau.n),
                      Tensor.wrap(r, o[3][0], self.rau.n, cfg.S), Tensor.wrap(r, o[4][0], self.rau.n, cfg.R),
                      Tensor.wrap(r, o[5][0], self.rau.n, cfg.R) }
      return self.output
    end
    function m:backward(inp, g)   -- g = {d_logits, d_do_pred|nil, d_attprob|nil, d_c, d_h}
      local o = {}
      for k = 1, 4 do o[k] = ffi.new('float*[1]') end
      check(C.rau_multimodal_backward(self.rau.h, self.i, ptr_of(inp[1]), ptr_of(inp[2]),
                                      ptr_of(inp[3]), ptr_of(inp[4]), ptr_of(g[1]), ptr_of(g[2]),
                                      ptr_of(g[3]), ptr_of(g[4]), ptr_of(g[5]), o[1], nil, o[3], o[4]))
      local r = self.rau                                    -- {d_q, (d_X dead, SS:579), d_c, d_h}
      self.gradInput = { Tensor.wrap(r, o[1][0], self.rau.n, Q), nil, Tensor.wrap(r, o[3][0], self.rau.n, cfg.R),
                         Tensor.wrap(r, o[4][0], self.rau.n, cfg.R) }
      return self.gradInput
    end
  elseif kind == 'criterion' then
    function m:forward(logits, y)
      local l = ffi.new('float[1]')
      check(C.rau_criterion_forward(self.rau.h, self.i, ptr_of(logits), ptr_of(y), l))
      return l[0]
    end
    function m:backward(logits, y, scale)
      local o = ffi.new('float*[1]')
      check(C.rau_criterion_backward(self.rau.h, self.i, ptr_of(logits), ptr_of(y), scale or 1, o))
      return Tensor.wrap(self.rau, o[0], self.rau.n, cfg.K)
    end
    -- the same criterion against an answer set in device memory: ids (RAU.IntTensor [B,G], 0 = empty entry) and
    -- w (RAU.Tensor [B,G]), or raw device pointers
    function m:forwardSet(logits, ids, w, G)
      local l = ffi.new('float[1]')
      check(C.rau_criterion_forward_set(self.rau.h, self.i, ptr_of(logits), G, ptr_of(ids), ptr_of(w), l))
      return l[0]
    end
    function m:backwardSet(logits, ids, w, G, scale)
      local o = ffi.new('float*[1]')
      check(C.rau_criterion_backward_set(self.rau.h, self.i, ptr_of(logits), G, ptr_of(ids), ptr_of(w), scale or 1, o))
      return Tensor.wrap(self.rau, o[0], self.rau.n, cfg.K)
    end
    -- the per-answer sigmoid criterion (BCE against soft targets): y = labels (RAU.IntTensor [B]), or y = nil and an
    -- answer set ids / w / G as in forwardSet
    function m:forwardBCE(logits, y, ids, w, G)
      local l = ffi.new('float[1]')
      check(C.rau_criterion_forward_bce(self.rau.h, self.i, ptr_of(logits), y and ptr_of(y) or nil, G or 0,
                                        ids and ptr_of(ids) or nil, w and ptr_of(w) or nil, l))
      return l[0]
    end
    function m:backwardBCE(logits, y, ids, w, G, scale)
      local o = ffi.new('float*[1]')
      check(C.rau_criterion_backward_bce(self.rau.h, self.i, ptr_of(logits), y and ptr_of(y) or nil, G or 0,
                                         ids and ptr_of(ids) or nil, w and ptr_of(w) or nil, scale or 1, o))
      return Tensor.wrap(self.rau, o[0], self.rau.n, cfg.K)
    end
  end
  function m:training() self.rau:training() end
  function m:evaluate() self.rau:evaluate() end
  function m:cuda() return self end
  function m:clone() return self end                 -- clones share parameters by construction
  function m:getParameters() return self.rau:flat(kind == 'embed' and 'embed' or kind == 'rnn' and 'rnn' or 'mult') end
  return m
end
function RAU:embedClone(t) return clone(self, 'embed', t) end
function RAU:rnnClone(t) return clone(self, 'rnn', t) end
function RAU:multimodalClone(h) return clone(self, 'multimodal', h) end
function RAU:criterion(h) return clone(self, 'criterion', h) end
-- criteria[h] against an answer set, without making the clone: loss / d_logits (see forwardSet / backwardSet)
function RAU:criterionForwardSet(h, logits, ids, w, G) return clone(self, 'criterion', h):forwardSet(logits, ids, w, G) end
function RAU:criterionBackwardSet(h, logits, ids, w, G, scale)
  return clone(self, 'criterion', h):backwardSet(logits, ids, w, G, scale)
end

return RAU

// rau_batch.hip -- how a batch reaches a context (include/rau.h: batch, 16-bit maps, image tables, feature
// bank, asynchronous upload) and how the step reads it back (batch_maps).
//
// A context has two batch slots (rau_ctx.h: BatchSlot); slot[cur_slot] is the resident batch and the only
// record of it.  There is ONE upload path with two front ends:
//   set_batch_sync  -- into the current slot, on the chain stream, from the caller's memory; synchronising;
//   set_batch_slot  -- into either slot, on the copy stream, from the slot's pinned staging; ordered against
//                      the steps by the slot's two events, made current by rau_use_batch.
// Both check the arguments (check_images, index_batch), describe the batch as one `Batch`, enqueue its copies
// (enqueue_batch) and record what the slot now holds (hold).
#include "rau_ctx.h"
#include "packed.h"

namespace {
// Host-side half of a batch hand-over: argument checks and the distinct-token index over the live
// positions (t < lens[b]) that makes the LookupTable gradient a fixed-order gather-sum.
// utok / ustart / upos must hold T*B, T*B + 1, T*B entries.
int index_batch(const rau_config& c, const int32_t* tokens, const int32_t* lens, const int32_t* labels,
                int32_t* utok, int32_t* ustart, int32_t* upos, int* max_len_out, int* nuniq_out) {
  int max_len = 0;
  for (int b = 0; b < c.B; ++b) {
    NEED(lens[b] >= 0 && lens[b] <= c.T, "lens[%d]=%d out of [0,%d]", b, lens[b], c.T);
    max_len = std::max(max_len, lens[b]);
  }
  for (size_t i = 0; i < (size_t)c.T * c.B; ++i)
    NEED(tokens[i] >= 1 && tokens[i] <= c.V, "token %d at %zu out of [1,%d]", tokens[i], i, c.V);
  if (labels)
    for (int b = 0; b < c.B; ++b)
      NEED(labels[b] >= 1 && labels[b] <= c.K, "labels[%d]=%d out of [1,%d]", b, labels[b], c.K);
  std::vector<std::pair<int32_t, int32_t>> pos;  // (token, position)
  for (int t = 0; t < max_len; ++t)
    for (int b = 0; b < c.B; ++b)
      if (t < lens[b]) pos.push_back({tokens[(size_t)t * c.B + b], t * c.B + b});
  std::sort(pos.begin(), pos.end());
  const size_t TB = (size_t)c.T * c.B;
  size_t nu = 0;
  for (size_t i = 0; i < pos.size(); ++i) {
    if (i == 0 || pos[i].first != pos[i - 1].first) {
      utok[nu] = pos[i].first;
      ustart[nu] = (int32_t)i;
      ++nu;
    }
    upos[i] = pos[i].second;
  }
  // pad to the maximum token count: a graph-captured embed_bwd launches T*B blocks, the surplus
  // ones see an empty range
  for (size_t i = nu; i < TB; ++i) utok[i] = 1;
  for (size_t i = nu; i <= TB; ++i) ustart[i] = (int32_t)pos.size();
  for (size_t i = pos.size(); i < TB; ++i) upos[i] = 0;
  *max_len_out = max_len;
  *nuniq_out = (int)nu;
  return RAU_OK;
}

// One batch on its way into a slot.  The first half is what the caller handed over; the asynchronous front end
// re-points it at the slot's pinned staging once the batch has been copied there.
struct Batch {
  const void* feats = nullptr;   // B maps, or the n_images maps of a table, of feat_type; null: a bank batch
  int feat_type = RAU_FEAT_F32;
  int n_images = 0;              // n_images == 0 with image_of == null is the plain batch; once check_images has
  const int32_t* image_of = nullptr;   // passed, n_images > 0 says "table"
  const int32_t *tokens = nullptr, *lens = nullptr, *labels = nullptr;
  const int32_t* bank_rows = nullptr;   // non-null: the table is bank[bank_rows]
  // packed batch (rau_set_batch_packed): feats holds pk_rows region rows [pk_rows][D], map i owns pk_counts[i] of
  // them; the maps (B of them, or the n_images of a table) are unpacked on the device
  const int32_t* pk_counts = nullptr;
  size_t pk_rows = 0;                   // sum of pk_counts (check_packed)
  const int32_t* pk_meta = nullptr;     // off[maps] | cnt[maps]
  const int32_t* pk_nreg = nullptr;     // [B] region counts per SAMPLE: pk_counts, or pk_counts[image_of]
  // ---- worked out on the way in
  const int32_t* bank_idx = nullptr;    // [2B], check_bank_rows
  const int32_t* img_block = nullptr;   // table batch: image_of | img_start | img_samples as the slot stores them (stage_table)
  bool bank_table = false;              // the upload gathers the table itself (wants_table)
  const int32_t *utok = nullptr, *ustart = nullptr, *upos = nullptr;   // index_batch
  int max_len = 0, nuniq = 0;
};

// image table of a batch: n_images in [1, B], every entry of the host index a row of the table
int check_table(const rau_config& c, int n_images, const int32_t* image_of) {
  NEED(image_of, "null image_of");
  NEED(n_images >= 1 && n_images <= c.B, "n_images=%d out of [1,%d]", n_images, c.B);
  for (int b = 0; b < c.B; ++b)
    NEED(image_of[b] >= 0 && image_of[b] < n_images, "image_of[%d]=%d out of [0,%d)", b, image_of[b], n_images);
  return RAU_OK;
}
// The sample lists of a table (rau_image_lists): a stable counting sort over image_of, so image i owns
// samples[start[i] .. start[i + 1]) in ascending sample order.  start has slots + 1 entries; the slots at and behind
// n_images are empty (start = n).  image_of has passed check_table.
void image_lists(int n, int n_images, const int32_t* image_of, int slots, int32_t* start, int32_t* samples) {
  std::fill(start, start + slots + 1, 0);
  for (int b = 0; b < n; ++b) ++start[image_of[b] + 1];
  for (int i = 0; i < n_images; ++i) start[i + 1] += start[i];
  for (int i = n_images + 1; i <= slots; ++i) start[i] = n;
  std::vector<int32_t> at(start, start + n_images);
  for (int b = 0; b < n; ++b) samples[at[image_of[b]]++] = b;
}
// A table batch's index block in the layout of BatchSlot::image_of_d: image_of [cap] | img_start [cap + 1] |
// img_samples [cap], the lists over all `cap` image slots (the per-image gradient pass is launched over the capacity)
size_t table_block_words(const rau_ctx* ctx) { return 3 * (size_t)ctx->cap + 1; }
void stage_table(const rau_ctx* ctx, int n_images, const int32_t* image_of, int32_t* block) {
  const int n = ctx->cfg.B, cap = ctx->cap;
  std::copy(image_of, image_of + n, block);
  std::fill(block + n, block + cap, 0);
  image_lists(n, n_images, image_of, cap, block + cap, block + 2 * (size_t)cap + 1);
  std::fill(block + 2 * (size_t)cap + 1 + n, block + table_block_words(ctx), 0);
}
// what the two bank entry points ask before anything else
int need_bank(const rau_ctx* ctx, const char* who, const int32_t* rows) {
  if (!ctx->bank) return fail(RAU_ERR_STATE, "%s: the context has no feature bank (rau_bank_create)", who);
  NEED(rows, "null bank_rows");
  return RAU_OK;
}
// bank batch: the table is valid, every row lies in the bank and has been written; fills
// idx[2B] = rows (padded with rows[0]) | rows[image_of[b]]
int check_bank_rows(rau_ctx* ctx, int n_images, const int32_t* rows, const int32_t* image_of, int32_t* idx) {
  const rau_config& c = ctx->cfg;
  if (int rc = check_table(c, n_images, image_of)) return rc;
  for (int n = 0; n < n_images; ++n)
    NEED(rows[n] >= 0 && rows[n] < ctx->bank_cap, "bank_rows[%d]=%d out of [0,%d)", n, rows[n], ctx->bank_cap);
  for (int n = 0; n < n_images; ++n)
    if (!ctx->bank_written[rows[n]])
      return fail(RAU_ERR_STATE, "bank_rows[%d]=%d has never been written (rau_bank_put)", n, rows[n]);
  for (int b = 0; b < c.B; ++b) {
    idx[b] = rows[b < n_images ? b : 0];
    idx[c.B + b] = rows[image_of[b]];
  }
  return RAU_OK;
}
int ensure_packed(rau_ctx* ctx, int si, bool pinned);   // (below, next to ensure_regions)
// packed batch: as many maps as samples unless an index names them, every count in [1, S]; *total = their sum
int check_packed(const rau_config& c, int n_maps, const int32_t* counts, const int32_t* image_of, size_t* total) {
  NEED(counts, "null counts");
  NEED(n_maps >= 1 && n_maps <= c.B, "n_maps=%d out of [1,%d]", n_maps, c.B);
  NEED(image_of || n_maps == c.B, "n_maps=%d without image_of: a plain batch has %d maps", n_maps, c.B);
  size_t sum = 0;
  for (int i = 0; i < n_maps; ++i) {
    NEED(counts[i] >= 1 && counts[i] <= c.S, "counts[%d]=%d out of [1,%d]", i, counts[i], c.S);
    sum += (size_t)counts[i];
  }
  *total = sum;
  return RAU_OK;
}
// meta[2 * maps] = exclusive prefix sums | counts; nreg[B] = the count of the map each sample looks at
void fill_packed(const rau_config& c, const Batch& b, int32_t* meta, int32_t* nreg) {
  const int maps = b.n_images > 0 ? b.n_images : c.B;
  int32_t off = 0;
  for (int i = 0; i < maps; ++i) {
    meta[i] = off;
    meta[maps + i] = b.pk_counts[i];
    off += b.pk_counts[i];
  }
  for (int s = 0; s < c.B; ++s) nreg[s] = b.pk_counts[b.image_of ? b.image_of[s] : s];
}
// the image half of a batch's argument checks; a bank batch's row index goes to idx[2B]
int check_images(rau_ctx* ctx, const Batch& b, int32_t* idx) {
  if (b.bank_rows) return check_bank_rows(ctx, b.n_images, b.bank_rows, b.image_of, idx);
  if (b.n_images != 0 || b.image_of) return check_table(ctx->cfg, b.n_images, b.image_of);
  return RAU_OK;
}
// A bank batch's table is wanted by the evaluate-mode forward only; a train-mode step gathers per-sample maps
// straight from the bank (batch_maps), and a later evaluate-mode forward gathers the table then.
bool wants_table(const rau_ctx* ctx, const Batch& b) { return b.bank_rows && ctx->mode == RAU_MODE_EVAL; }

// first table batch of a slot: its device index (and pinned staging of it on the asynchronous path) and the
// ctx's buffer of expanded per-sample maps
int ensure_table(rau_ctx* ctx, int si, bool pinned, bool bank) {
  const rau_config& c = ctx->cfg;
  const size_t cap = (size_t)ctx->cap;   // sized once, for the capacity; contents are dense in the current size
  BatchSlot& s = ctx->slot[si];
  if (bank && !s.bank_idx_d)
    if (int rc = dalloc(ctx, &s.bank_idx_d, 2 * cap)) return rc;
  if (bank && pinned && !s.bank_idx_h) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, 2 * cap * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(bank index staging): %s", hipGetErrorString(e));
    s.bank_idx_h = static_cast<int32_t*>(h);
  }
  if (!s.image_of_d) {
    if (int rc = dalloc(ctx, &s.image_of_d, table_block_words(ctx))) return rc;
    s.img_start_d = s.image_of_d + cap;
    s.img_samples_d = s.img_start_d + cap + 1;
  }
  if (!ctx->feats_x)
    if (int rc = dalloc(ctx, &ctx->feats_x, cap * c.D * ctx->Sp)) return rc;
  if (pinned && !s.image_of_h) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, table_block_words(ctx) * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(image index staging): %s", hipGetErrorString(e));
    s.image_of_h = static_cast<int32_t*>(h);
  }
  return RAU_OK;
}

// what the asynchronous path adds to rau_create's slot 0: slot 1's device buffers, pinned staging and events
// for both slots, the copy stream
int ensure_async(rau_ctx* ctx) {
  if (ctx->async_ready) return RAU_OK;
  const rau_config& c = ctx->cfg;
  // Sized for the capacity, and the staging's sub-arrays START where the capacity puts them; what a batch of the
  // current size n writes into each of them is dense in n ([n,D,S], [T,n], [n], [n]).
  const size_t B = (size_t)ctx->cap;
  const size_t TB = (size_t)c.T * B, nf = B * c.D * c.S;
  BatchSlot& s1 = ctx->slot[1];
  if (int rc = dalloc(ctx, &s1.feats, B * c.D * ctx->Sp)) return rc;
  if (int rc = dalloc(ctx, &s1.tokens, TB)) return rc;
  if (int rc = dalloc(ctx, &s1.lens_d, B)) return rc;
  if (int rc = dalloc(ctx, &s1.labels_d, B)) return rc;
  if (int rc = dalloc(ctx, &s1.utok, TB)) return rc;
  if (int rc = dalloc(ctx, &s1.ustart, TB + 1)) return rc;
  if (int rc = dalloc(ctx, &s1.upos, TB)) return rc;
  for (BatchSlot& s : ctx->slot) {
    // one pinned block per slot: feats | tokens | lens | labels | utok | ustart | upos
    const size_t words = nf + TB + 2 * B + TB + (TB + 1) + TB;
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, words * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(batch staging, %zu bytes): %s", words * 4,
                                     hipGetErrorString(e));
    s.feats_h = static_cast<float*>(h);
    s.tokens_h = reinterpret_cast<int32_t*>(s.feats_h + nf);
    s.lens_p = s.tokens_h + TB;
    s.labels_h = s.lens_p + B;
    s.utok_h = s.labels_h + B;
    s.ustart_h = s.utok_h + TB;
    s.upos_h = s.ustart_h + TB + 1;
    HIPC(hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming));
  }
  int plo = 0, phi = 0;
  hipDeviceGetStreamPriorityRange(&plo, &phi);
  HIPC(hipStreamCreateWithPriority(&ctx->stc, hipStreamNonBlocking, plo));
  ctx->async_ready = true;
  return RAU_OK;
}

// H2D copies of batch `b` into slot si's device buffers, enqueued on `st`: one more upload into that slot.
int enqueue_batch(rau_ctx* ctx, hipStream_t st, int si, const Batch& b) {
  const rau_config& c = ctx->cfg;
  const BatchSlot& d = ctx->slot[si];
  const size_t TB = (size_t)c.T * c.B, es = feat_elem_bytes(b.feat_type);
  const size_t maps = b.n_images > 0 ? (size_t)b.n_images : (size_t)c.B;   // only these cross the bus
  ++ctx->slot_serial[si];
  if (b.n_images > 0)   // the index and the sample lists built from it: one block
    HIPC(hipMemcpyAsync(d.image_of_d, b.img_block, table_block_words(ctx) * 4, hipMemcpyHostToDevice, st));
  // pitched rows of another element size (4, 2 or 1 bytes) leave data in this type's pad columns: zero the
  // whole buffer first, on any change of type
  // (a packed batch of B maps writes every pad column itself)
  if ((b.feats || b.bank_idx) && ctx->Sp != c.S && b.feat_type != d.held.feat_type &&
      !(b.pk_counts && maps == (size_t)c.B))
    HIPC(hipMemsetAsync(d.feats, 0, (size_t)c.B * c.D * ctx->Sp * sizeof(float), st));
  // bank batch (feats == nullptr): only the two row indices cross the bus; the table is gathered inside device
  // memory behind them, whole maps with their (zero) pad columns
  if (b.bank_idx) {
    HIPC(hipMemcpyAsync(d.bank_idx_d, b.bank_idx, 2 * (size_t)c.B * 4, hipMemcpyHostToDevice, st));
    if (b.bank_table) {
      const size_t map_bytes = (size_t)c.D * ctx->Sp * es;
      RUNS(st, "bank_gather", 0, 2.0 * b.n_images * map_bytes,
           bank_gather(st, b.n_images, map_bytes, ctx->bank, ctx->bank_cap, d.bank_idx_d, d.feats));
    }
  }
  if (b.pk_counts) {
    // packed rows: only sum(counts) * D elements cross the bus; the unpack writes whole maps, pad columns included,
    // and the counts become the batch's region counts
    HIPC(hipMemcpyAsync(d.pk_rows_d, b.feats, b.pk_rows * c.D * es, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d.pk_meta_d, b.pk_meta, 2 * maps * 4, hipMemcpyHostToDevice, st));
    RUNS(st, "unpack_regions", 0, (double)(b.pk_rows * c.D + maps * c.D * ctx->Sp) * es,
         unpack_regions(st, (int)maps, c.D, c.S, ctx->Sp, d.pk_rows_d, b.pk_rows, d.pk_meta_d, d.pk_meta_d + maps,
                        d.feats, b.feat_type, b.feat_type));
    HIPC(hipMemcpyAsync(d.nreg_d, b.pk_nreg, (size_t)c.B * 4, hipMemcpyHostToDevice, st));
  } else if (b.feats && ctx->Sp == c.S)   // dense on both sides: one linear copy (a DMA-engine transfer, no blit kernel)
    HIPC(hipMemcpyAsync(d.feats, b.feats, maps * c.D * c.S * es, hipMemcpyHostToDevice, st));
  else if (b.feats)   // rows of S positions into rows of Sp (pad columns stay zero)
    HIPC(hipMemcpy2DAsync(d.feats, (size_t)ctx->Sp * es, b.feats, (size_t)c.S * es, (size_t)c.S * es,
                          maps * c.D, hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(d.tokens, b.tokens, TB * 4, hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(d.lens_d, b.lens, (size_t)c.B * 4, hipMemcpyHostToDevice, st));
  if (b.labels) HIPC(hipMemcpyAsync(d.labels_d, b.labels, (size_t)c.B * 4, hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(d.utok, b.utok, TB * 4, hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(d.upos, b.upos, TB * 4, hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(d.ustart, b.ustart, (TB + 1) * 4, hipMemcpyHostToDevice, st));
  return RAU_OK;
}
// slot si now holds batch `b`
void hold(rau_ctx* ctx, int si, const Batch& b) {
  BatchDesc& d = ctx->slot[si].held;
  d.feat_type = b.feat_type;
  d.n_images = b.n_images;
  d.bank = b.bank_rows != nullptr;
  d.table_ok = b.bank_table;
  d.lens.assign(b.lens, b.lens + ctx->cfg.B);
  d.max_len = b.max_len;
  d.nuniq = b.nuniq;
  d.have = true;
  d.have_labels = b.labels != nullptr;
  d.ans_G = 0;   // an answer set belongs to the batch it was given to
  d.regions = b.pk_counts != nullptr;   // ... and so do region counts (a packed batch brings its own)
  d.att_targets = false;   // ... and attention targets
  d.sample_w = false;      // ... and per-sample loss weights
  d.cand_C = 0;            // ... and multiple-choice candidates
  d.question = false;      // ... and the caller's question state
  d.state = false;         // ... and the caller's initial state (the next forward clears the rows itself)
  d.att_bias = false;      // ... and the caller's attention bias
}

// rau_set_batch_images, or (b.bank_rows) the same batch with its table drawn from the bank
int set_batch_sync(rau_ctx* ctx, Batch b) {
  const rau_config& c = ctx->cfg;
  std::vector<int32_t> bidx(b.bank_rows ? 2 * (size_t)c.B : 0);
  if (b.pk_counts)
    if (int rc = check_packed(c, b.n_images ? b.n_images : c.B, b.pk_counts, b.image_of, &b.pk_rows)) return rc;
  if (int rc = check_images(ctx, b, bidx.data())) return rc;
  const size_t TB = (size_t)c.T * c.B;
  std::vector<int32_t> utok(TB), ustart(TB + 1), upos(TB);
  if (int rc = index_batch(c, b.tokens, b.lens, b.labels, utok.data(), ustart.data(), upos.data(), &b.max_len,
                           &b.nuniq))
    return rc;
  b.utok = utok.data(); b.ustart = ustart.data(); b.upos = upos.data();
  b.bank_idx = b.bank_rows ? bidx.data() : nullptr;
  b.bank_table = wants_table(ctx, b);
  const int si = ctx->cur_slot;   // slot 0 unless rau_use_batch switched
  BatchSlot& s = ctx->slot[si];
  std::vector<int32_t> tblock;
  if (b.n_images) {
    if (int rc = ensure_table(ctx, si, false, b.bank_rows != nullptr)) return rc;
    tblock.resize(table_block_words(ctx));
    stage_table(ctx, b.n_images, b.image_of, tblock.data());
    b.img_block = tblock.data();
  }
  std::vector<int32_t> pmeta, pnreg;
  if (b.pk_counts) {
    if (int rc = ensure_packed(ctx, si, false)) return rc;
    pmeta.resize(2 * (size_t)c.B);
    pnreg.resize((size_t)c.B);
    fill_packed(c, b, pmeta.data(), pnreg.data());
    b.pk_meta = pmeta.data();
    b.pk_nreg = pnreg.data();
  }
  if (s.upload_pending)   // an async upload into the same buffers
    HIPC(hipStreamWaitEvent(ctx->st, s.uploaded, 0));
  if (int rc = enqueue_batch(ctx, ctx->st, si, b)) return rc;
  HIPC(hipStreamSynchronize(ctx->st));   // the caller's (pageable) buffers are free on return
  s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  hold(ctx, si, b);
  drop_forward(ctx);
  return RAU_OK;
}

// rau_set_batch_async_images, or (b.bank_rows) the same batch with its table drawn from the bank: nothing is
// written to the slot's feature staging and no feature byte crosses the bus
int set_batch_slot(rau_ctx* ctx, int slot, Batch b, int has_labels) {
  NEED(slot == 0 || slot == 1, "rau_set_batch_async: slot %d (0 or 1)", slot);
  const rau_config& c = ctx->cfg;
  std::vector<int32_t> bidx(b.bank_rows ? 2 * (size_t)c.B : 0);
  if (b.pk_counts)
    if (int rc = check_packed(c, b.n_images ? b.n_images : c.B, b.pk_counts, b.image_of, &b.pk_rows)) return rc;
  if (int rc = check_images(ctx, b, bidx.data())) return rc;
  if (int rc = ensure_async(ctx)) return rc;
  if (b.n_images)
    if (int rc = ensure_table(ctx, slot, true, b.bank_rows != nullptr)) return rc;
  if (b.pk_counts)
    if (int rc = ensure_packed(ctx, slot, true)) return rc;
  BatchSlot& s = ctx->slot[slot];
  if (slot == ctx->cur_slot && ctx->fwd.done)
    return fail(RAU_ERR_STATE, "rau_set_batch_async: slot %d is the current batch of a forward pass whose "
                "backward has not run; upload into the other slot", slot);
  const size_t TB = (size_t)c.T * c.B;
  const size_t nf = b.pk_counts ? b.pk_rows * c.D : (size_t)(b.n_images ? b.n_images : c.B) * c.D * c.S;
  // The slot's previous upload may not have left its pinned staging yet: index_batch below rewrites the
  // pinned index arrays in every case, and the memcpys rewrite the rest, so wait for it either way.
  // (A caller that refills the staging IN PLACE must call rau_batch_slot(slot) before every refill:
  // that call performs the same wait before the caller's own writes -- include/rau.h.)
  if (s.upload_pending) {
    HIPC(hipEventSynchronize(s.uploaded));
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  }
  // NULL = the caller has filled the slot's pinned staging in place (rau_batch_slot)
  if (b.feats && b.feats != s.feats_h) std::memcpy(s.feats_h, b.feats, nf * feat_elem_bytes(b.feat_type));
  if (b.tokens && b.tokens != s.tokens_h) std::memcpy(s.tokens_h, b.tokens, TB * 4);
  if (b.lens && b.lens != s.lens_p) std::memcpy(s.lens_p, b.lens, (size_t)c.B * 4);
  if (b.labels && b.labels != s.labels_h) std::memcpy(s.labels_h, b.labels, (size_t)c.B * 4);
  if (b.n_images) stage_table(ctx, b.n_images, b.image_of, s.image_of_h);
  if (b.bank_rows) std::memcpy(s.bank_idx_h, bidx.data(), 2 * (size_t)c.B * 4);
  if (b.pk_counts) {   // (before image_of is re-pointed: both arrays still are the caller's)
    fill_packed(c, b, s.pk_meta_h, s.nreg_h);
    b.pk_meta = s.pk_meta_h;
    b.pk_nreg = s.nreg_h;
  }
  // from here on the batch is the staging's
  b.feats = b.bank_rows ? nullptr : s.feats_h;
  b.tokens = s.tokens_h;
  b.lens = s.lens_p;
  b.labels = (b.labels || has_labels) ? s.labels_h : nullptr;
  b.image_of = b.img_block = s.image_of_h;
  b.bank_idx = b.bank_rows ? s.bank_idx_h : nullptr;
  b.bank_table = wants_table(ctx, b);
  b.utok = s.utok_h; b.ustart = s.ustart_h; b.upos = s.upos_h;
  if (int rc = index_batch(c, b.tokens, b.lens, b.labels, s.utok_h, s.ustart_h, s.upos_h, &b.max_len, &b.nuniq))
    return rc;
  // device side: the slot's buffers may still be read by the last step that used them
  if (slot == ctx->cur_slot) {
    HIPC(hipEventRecord(s.consumed, ctx->st));
    s.consumed_valid = true;
  }
  if (s.consumed_valid) HIPC(hipStreamWaitEvent(ctx->stc, s.consumed, 0));
  if (int rc = enqueue_batch(ctx, ctx->stc, slot, b)) return rc;
  HIPC(hipEventRecord(s.uploaded, ctx->stc));
  s.upload_pending = true;
  if (b.pk_counts) s.reg_pending = true;   // a copy out of nreg_h is behind this record
  hold(ctx, slot, b);
  if (slot == ctx->cur_slot) {   // re-filled in place: the next forward waits for the copies
    drop_forward(ctx);
    HIPC(hipStreamWaitEvent(ctx->st, s.uploaded, 0));
  }
  return RAU_OK;
}

// first answer set of a slot: its device block ids | w | score (each [capacity][kMaxAnswers]) and the pinned
// staging the copies read
int ensure_answers(rau_ctx* ctx, int si) {
  BatchSlot& s = ctx->slot[si];
  const size_t n = (size_t)ctx->cap * kMaxAnswers;
  if (!s.ans_ids_d) {
    int32_t* d = nullptr;
    if (int rc = dalloc(ctx, &d, 3 * n)) return rc;
    s.ans_ids_d = d;
    s.ans_w_d = reinterpret_cast<float*>(d + n);
    s.ans_score_d = reinterpret_cast<float*>(d + 2 * n);
    // dalloc clears the block on the chain stream; the slot form copies into it on the copy stream.  Once per slot.
    HIPC(hipStreamSynchronize(ctx->st));
  }
  if (!s.ans_h) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, 3 * n * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(answer staging): %s", hipGetErrorString(e));
    s.ans_h = static_cast<int32_t*>(h);
  }
  return RAU_OK;
}

// first region counts of a slot: the device array [capacity] the attention kernels read and the pinned staging the
// slot form copies from
int ensure_regions(rau_ctx* ctx, int si) {
  BatchSlot& s = ctx->slot[si];
  if (!s.nreg_d) {
    if (int rc = dalloc(ctx, &s.nreg_d, (size_t)ctx->cap)) return rc;
    // dalloc clears the array on the chain stream; the slot form copies into it on the copy stream.  Once per slot.
    HIPC(hipStreamSynchronize(ctx->st));
  }
  if (!s.nreg_h) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, (size_t)ctx->cap * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(region count staging): %s", hipGetErrorString(e));
    s.nreg_h = static_cast<int32_t*>(h);
  }
  return RAU_OK;
}

// first sample weights of a slot: the device array [capacity] the loss kernels read and the pinned staging the copies
// read
int ensure_sample_weights(rau_ctx* ctx, int si) {
  BatchSlot& s = ctx->slot[si];
  if (!s.sw_d) {
    if (int rc = dalloc(ctx, &s.sw_d, (size_t)ctx->cap)) return rc;
    // dalloc clears the array on the chain stream; the slot form copies into it on the copy stream.  Once per slot.
    HIPC(hipStreamSynchronize(ctx->st));
  }
  if (!s.sw_h) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, (size_t)ctx->cap * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(sample weight staging): %s", hipGetErrorString(e));
    s.sw_h = static_cast<float*>(h);
  }
  return RAU_OK;
}

// first candidate list of a slot: the device array [capacity][kMaxCandidates] the criterion head reads and the pinned
// staging the copies read
int ensure_candidates(rau_ctx* ctx, int si) {
  BatchSlot& s = ctx->slot[si];
  const size_t n = (size_t)ctx->cap * kMaxCandidates;
  if (!s.cand_d) {
    if (int rc = dalloc(ctx, &s.cand_d, n)) return rc;
    // dalloc clears the array on the chain stream; the slot form copies into it on the copy stream.  Once per slot.
    HIPC(hipStreamSynchronize(ctx->st));
  }
  if (!s.cand_h) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, n * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(candidate staging): %s", hipGetErrorString(e));
    s.cand_h = static_cast<int32_t*>(h);
  }
  return RAU_OK;
}

// first attention targets of a slot: the device block [capacity][Sp] the supervision kernels read (pad columns are
// never written: they keep dalloc's zeros) and the pinned staging [capacity][S] the copies read
int ensure_att_targets(rau_ctx* ctx, int si) {
  BatchSlot& s = ctx->slot[si];
  if (!s.att_t_d) {
    if (int rc = dalloc(ctx, &s.att_t_d, (size_t)ctx->cap * ctx->Sp)) return rc;
    // dalloc clears the block on the chain stream; the slot form copies into it on the copy stream.  Once per slot.
    HIPC(hipStreamSynchronize(ctx->st));
  }
  if (!s.att_t_h) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, (size_t)ctx->cap * ctx->cfg.S * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(attention target staging): %s", hipGetErrorString(e));
    s.att_t_h = static_cast<float*>(h);
  }
  return RAU_OK;
}

// first packed batch of a slot: the device staging of the raw rows (sized for the capacity and the widest element),
// the off | cnt arrays, the region counts; pinned staging of the small arrays on the asynchronous path
int ensure_packed(rau_ctx* ctx, int si, bool pinned) {
  const rau_config& c = ctx->cfg;
  const size_t cap = (size_t)ctx->cap;
  BatchSlot& s = ctx->slot[si];
  if (int rc = ensure_regions(ctx, si)) return rc;
  if (!s.pk_meta_d)
    if (int rc = dalloc(ctx, &s.pk_meta_d, 2 * cap)) return rc;
  if (pinned && !s.pk_meta_h) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, 2 * cap * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(packed offsets staging): %s", hipGetErrorString(e));
    s.pk_meta_h = static_cast<int32_t*>(h);
  }
  if (!s.pk_rows_d) {
    float* d = nullptr;   // (not scratch: every packed batch overwrites what it reads)
    if (int rc = dalloc(ctx, &d, cap * c.S * c.D, false)) {
      (void)hipGetLastError();   // the failed allocation is reported here, not by the next launch
      return rc;
    }
    s.pk_rows_d = d;
    // dalloc clears the block on the chain stream; the slot form copies into it on the copy stream.  Once per slot.
    HIPC(hipStreamSynchronize(ctx->st));
  }
  return RAU_OK;
}

// Every enqueued reader of the bank (the gathers: copy stream and chain stream) has finished.
int bank_quiesce(rau_ctx* ctx) {
  if (ctx->stc) HIPC(hipStreamSynchronize(ctx->stc));
  HIPC(hipStreamSynchronize(ctx->st));
  return RAU_OK;
}
// rau_bank_put's two pinned staging halves with their events and, where a kernel reads the chunk (`stage`), the
// device block it is copied to
int ensure_bank_staging(rau_ctx* ctx, bool stage) {
  const rau_config& c = ctx->cfg;
  if (!ctx->bank_chunk) {   // staging sized for f32 sources: 32 MiB, at least one map
    const size_t chunk = std::max<size_t>((size_t)32 << 20, (size_t)c.D * c.S * 4);
    for (int k = 0; k < 2; ++k) {
      if (!ctx->bank_pin[k]) {
        hipError_t e = hipHostMalloc(&ctx->bank_pin[k], chunk, hipHostMallocDefault);
        if (e != hipSuccess) {
          ctx->bank_pin[k] = nullptr;
          return fail(RAU_ERR_NOMEM, "rau_bank_put: hipHostMalloc(%zu bytes staging): %s", chunk, hipGetErrorString(e));
        }
      }
      if (!ctx->bank_ev[k]) HIPC(hipEventCreateWithFlags(&ctx->bank_ev[k], hipEventDisableTiming));
    }
    ctx->bank_chunk = chunk;
  }
  if (stage && !ctx->bank_stage) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&ctx->bank_stage), ctx->bank_chunk);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      ctx->bank_stage = nullptr;
      return fail(RAU_ERR_NOMEM, "rau_bank_put: hipMalloc(%zu bytes staging): %s", ctx->bank_chunk, hipGetErrorString(e));
    }
  }
  return RAU_OK;
}
constexpr int kBankPackMaps = 4096;   // maps per chunk of rau_bank_put_packed (their off | cnt arrays)
size_t bank_map_bytes(const rau_ctx* ctx) {
  return (size_t)ctx->cfg.D * ctx->Sp * feat_elem_bytes(ctx->bank_type);
}
}  // namespace

int batch_maps(rau_ctx* ctx, const float** maps) {
  const BatchSlot& bs = cur_batch(ctx);
  *maps = bs.feats;
  if (!bs.held.n_images) return RAU_OK;
  const rau_config& c = ctx->cfg;
  *maps = ctx->feats_x;
  // a captured launch gathers on every replay (the table and the index live in device memory); otherwise once
  // per upload into the slot
  if (!ctx->capturing && ctx->x_valid && ctx->x_slot == ctx->cur_slot &&
      ctx->x_serial == ctx->slot_serial[ctx->cur_slot])
    return RAU_OK;
  const size_t map_bytes = (size_t)c.D * ctx->Sp * feat_elem_bytes(bs.held.feat_type);
  hipStream_t st = ctx->st;
  if (bs.held.bank)   // one pass with the composed index rows[image_of[b]] (the second half of the slot's bank index)
    RUN("bank_gather", 0, 2.0 * c.B * map_bytes,
        bank_gather(st, c.B, map_bytes, ctx->bank, ctx->bank_cap, bs.bank_idx_d + c.B, ctx->feats_x));
  else
    RUN("expand_features", 0, 2.0 * c.B * map_bytes,
        expand_features(st, c.B, map_bytes, bs.feats, bs.image_of_d, ctx->feats_x));
  ctx->x_valid = true;
  ctx->x_slot = ctx->cur_slot;
  ctx->x_serial = ctx->slot_serial[ctx->cur_slot];
  return RAU_OK;
}

extern "C" {

// ------------------------------------------------------------------ batch
int rau_set_batch(rau_ctx* ctx, const float* feats, const int32_t* tokens, const int32_t* lens,
                  const int32_t* labels) {
  return rau_set_batch_typed(ctx, feats, RAU_FEAT_F32, tokens, lens, labels);
}

int rau_set_batch_typed(rau_ctx* ctx, const void* feats, int feat_type, const int32_t* tokens,
                        const int32_t* lens, const int32_t* labels) {
  return rau_set_batch_images(ctx, feats, feat_type, 0, nullptr, tokens, lens, labels);
}

// n_images == 0 with image_of == NULL is the plain batch (what rau_set_batch_typed passes)
int rau_set_batch_images(rau_ctx* ctx, const void* feats, int feat_type, int n_images, const int32_t* image_of,
                         const int32_t* tokens, const int32_t* lens, const int32_t* labels) {
  NEED(ctx && tokens && lens, "null argument");
  NEED(feat_type_ok(feat_type), "rau_set_batch: feat_type %d (" RAU_FEAT_TYPE_LIST ")", feat_type);
  return set_batch_sync(ctx, Batch{feats, feat_type, n_images, image_of, tokens, lens, labels, nullptr});
}

// rau_set_batch with the maps already in device memory (a producer in front of the library: rau_set_feat_grad).
// One device-to-device copy on the chain stream, re-pitching where S % 4 != 0; the index arrays go through pinned
// staging of the ctx (two halves, alternated like the hop weights'), so nothing here waits for the device.
// n_images > 0: feats_dev is an image table of that many maps and image_of names each sample's (rau_set_batch_dev_images).
static int set_batch_dev(rau_ctx* ctx, const char* who, const float* feats_dev, int n_images, const int32_t* image_of,
                         const int32_t* tokens, const int32_t* lens, const int32_t* labels) {
  NEED(ctx && feats_dev && tokens && lens, "null argument");
  if (ctx->capturing) return fail(RAU_ERR_STATE, "%s: a step is being captured", who);
  const rau_config& c = ctx->cfg;
  if (n_images != 0 || image_of)
    if (int rc = check_table(c, n_images, image_of)) return rc;
  const size_t TBc = (size_t)c.T * ctx->cap, TB = (size_t)c.T * c.B, Bc = (size_t)ctx->cap;
  // tokens | lens | labels | utok | ustart | upos | a table's index block
  const size_t words = TBc + 2 * Bc + TBc + (TBc + 1) + TBc + table_block_words(ctx);
  const int si = ctx->cur_slot;
  if (n_images)
    if (int rc = ensure_table(ctx, si, false, false)) return rc;
  const int sl = (ctx->bdev_slot ^= 1);
  if (!ctx->bdev_h[sl]) {
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, words * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RAU_ERR_NOMEM, "hipHostMalloc(batch index staging): %s", hipGetErrorString(e));
    ctx->bdev_h[sl] = static_cast<int32_t*>(h);
    HIPC(hipEventCreateWithFlags(&ctx->bdev_ev[sl], hipEventDisableTiming));
  } else {
    HIPC(hipEventSynchronize(ctx->bdev_ev[sl]));   // the copies out of this half, two calls ago
  }
  int32_t* tok_h = ctx->bdev_h[sl];
  int32_t* lens_h = tok_h + TBc;
  int32_t* lab_h = lens_h + Bc;
  int32_t* utok_h = lab_h + Bc;
  int32_t* ustart_h = utok_h + TBc;
  int32_t* upos_h = ustart_h + TBc + 1;
  int32_t* img_h = upos_h + TBc;
  std::memcpy(tok_h, tokens, TB * 4);
  std::memcpy(lens_h, lens, (size_t)c.B * 4);
  if (labels) std::memcpy(lab_h, labels, (size_t)c.B * 4);
  Batch b{nullptr, RAU_FEAT_F32, n_images, nullptr, tok_h, lens_h, labels ? lab_h : nullptr, nullptr};
  if (int rc = index_batch(c, b.tokens, b.lens, b.labels, utok_h, ustart_h, upos_h, &b.max_len, &b.nuniq)) return rc;
  b.utok = utok_h; b.ustart = ustart_h; b.upos = upos_h;
  if (n_images) {
    stage_table(ctx, n_images, image_of, img_h);
    b.image_of = b.img_block = img_h;
  }
  const size_t maps = n_images ? (size_t)n_images : (size_t)c.B;
  BatchSlot& s = ctx->slot[si];
  hipStream_t st = ctx->st;
  if (s.upload_pending) HIPC(hipStreamWaitEvent(st, s.uploaded, 0));   // an async upload into the same buffers
  if (ctx->Sp == c.S) {
    HIPC(hipMemcpyAsync(s.feats, feats_dev, maps * c.D * c.S * 4, hipMemcpyDeviceToDevice, st));
  } else {
    // rows of S floats into rows of Sp; another element type's rows leave data in the pad columns: cleared first
    if (s.held.feat_type != RAU_FEAT_F32)
      HIPC(hipMemsetAsync(s.feats, 0, (size_t)c.B * c.D * ctx->Sp * sizeof(float), st));
    HIPC(hipMemcpy2DAsync(s.feats, (size_t)ctx->Sp * 4, feats_dev, (size_t)c.S * 4, (size_t)c.S * 4,
                          maps * c.D, hipMemcpyDeviceToDevice, st));
  }
  if (int rc = enqueue_batch(ctx, st, si, b)) return rc;   // (feats == NULL: the index arrays only)
  HIPC(hipEventRecord(ctx->bdev_ev[sl], st));
  s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  hold(ctx, si, b);
  drop_forward(ctx);
  return RAU_OK;
}
int rau_set_batch_dev(rau_ctx* ctx, const float* feats_dev, const int32_t* tokens, const int32_t* lens,
                      const int32_t* labels) {
  return set_batch_dev(ctx, "rau_set_batch_dev", feats_dev, 0, nullptr, tokens, lens, labels);
}
int rau_set_batch_dev_images(rau_ctx* ctx, const float* table_dev, int n_images, const int32_t* image_of,
                             const int32_t* tokens, const int32_t* lens, const int32_t* labels) {
  NEED(ctx, "null ctx");
  NEED(image_of, "rau_set_batch_dev_images: null image_of");
  return set_batch_dev(ctx, "rau_set_batch_dev_images", table_dev, n_images, image_of, tokens, lens, labels);
}

// host-only diagnostic: the lists stage_table builds, for the n_images images alone
int rau_image_lists(int n, int n_images, const int32_t* image_of, int32_t* start, int32_t* samples) {
  NEED(image_of && start && samples, "rau_image_lists: null argument");
  NEED(n >= 1, "rau_image_lists: n=%d", n);
  NEED(n_images >= 1 && n_images <= n, "rau_image_lists: n_images=%d out of [1,%d]", n_images, n);
  for (int b = 0; b < n; ++b)
    NEED(image_of[b] >= 0 && image_of[b] < n_images, "rau_image_lists: image_of[%d]=%d out of [0,%d)", b, image_of[b],
         n_images);
  image_lists(n, n_images, image_of, n_images, start, samples);
  return RAU_OK;
}

int rau_set_batch_bank(rau_ctx* ctx, int n_images, const int32_t* bank_rows, const int32_t* image_of,
                       const int32_t* tokens, const int32_t* lens, const int32_t* labels) {
  NEED(ctx && tokens && lens, "null argument");
  if (int rc = need_bank(ctx, "rau_set_batch_bank", bank_rows)) return rc;
  return set_batch_sync(ctx, Batch{nullptr, ctx->bank_type, n_images, image_of, tokens, lens, labels, bank_rows});
}

// n_maps maps of counts[i] rows each; image_of == NULL: the plain batch, one map per sample
int rau_set_batch_packed(rau_ctx* ctx, const void* rows, int feat_type, int n_maps, const int32_t* counts,
                         const int32_t* image_of, const int32_t* tokens, const int32_t* lens, const int32_t* labels) {
  NEED(ctx && rows && tokens && lens, "null argument");
  NEED(feat_type_ok(feat_type), "rau_set_batch_packed: feat_type %d (" RAU_FEAT_TYPE_LIST ")", feat_type);
  NEED(counts, "rau_set_batch_packed: null counts");
  NEED(n_maps >= 1 && n_maps <= ctx->cfg.B, "rau_set_batch_packed: n_maps=%d out of [1,%d]", n_maps, ctx->cfg.B);
  NEED(image_of || n_maps == ctx->cfg.B, "rau_set_batch_packed: n_maps=%d without image_of (a plain batch has %d maps)",
       n_maps, ctx->cfg.B);
  return set_batch_sync(ctx, Batch{rows, feat_type, image_of ? n_maps : 0, image_of, tokens, lens, labels, nullptr,
                                   counts});
}

int rau_batch_slot(rau_ctx* ctx, int slot, float** feats_host, int32_t** tokens_host,
                   int32_t** lens_host, int32_t** labels_host) {
  NEED(ctx, "null ctx");
  NEED(slot == 0 || slot == 1, "rau_batch_slot: slot %d (0 or 1)", slot);
  if (int rc = ensure_async(ctx)) return rc;
  BatchSlot& s = ctx->slot[slot];
  if (s.upload_pending) {   // the caller is about to overwrite the staging: its last copy must have left
    HIPC(hipEventSynchronize(s.uploaded));
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  }
  if (feats_host) *feats_host = s.feats_h;
  if (tokens_host) *tokens_host = s.tokens_h;
  if (lens_host) *lens_host = s.lens_p;
  if (labels_host) *labels_host = s.labels_h;
  return RAU_OK;
}

int rau_set_batch_async(rau_ctx* ctx, int slot, const float* feats, const int32_t* tokens,
                        const int32_t* lens, const int32_t* labels, int has_labels) {
  return rau_set_batch_async_typed(ctx, slot, feats, RAU_FEAT_F32, tokens, lens, labels, has_labels);
}

int rau_set_batch_async_typed(rau_ctx* ctx, int slot, const void* feats, int feat_type,
                              const int32_t* tokens, const int32_t* lens, const int32_t* labels,
                              int has_labels) {
  return rau_set_batch_async_images(ctx, slot, feats, feat_type, 0, nullptr, tokens, lens, labels, has_labels);
}

// n_images == 0 with image_of == NULL is the plain batch (what rau_set_batch_async_typed passes)
int rau_set_batch_async_images(rau_ctx* ctx, int slot, const void* feats, int feat_type, int n_images,
                               const int32_t* image_of, const int32_t* tokens, const int32_t* lens,
                               const int32_t* labels, int has_labels) {
  NEED(ctx, "null ctx");
  NEED(feat_type_ok(feat_type), "rau_set_batch_async: feat_type %d (" RAU_FEAT_TYPE_LIST ")", feat_type);
  return set_batch_slot(ctx, slot, Batch{feats, feat_type, n_images, image_of, tokens, lens, labels, nullptr},
                        has_labels);
}

int rau_set_batch_async_bank(rau_ctx* ctx, int slot, int n_images, const int32_t* bank_rows,
                             const int32_t* image_of, const int32_t* tokens, const int32_t* lens,
                             const int32_t* labels, int has_labels) {
  NEED(ctx, "null ctx");
  if (int rc = need_bank(ctx, "rau_set_batch_async_bank", bank_rows)) return rc;
  return set_batch_slot(ctx, slot,
                        Batch{nullptr, ctx->bank_type, n_images, image_of, tokens, lens, labels, bank_rows},
                        has_labels);
}

// rows == NULL: the slot's pinned staging already holds the sum(counts) * D elements at its start
int rau_set_batch_async_packed(rau_ctx* ctx, int slot, const void* rows, int feat_type, int n_maps,
                               const int32_t* counts, const int32_t* image_of, const int32_t* tokens,
                               const int32_t* lens, const int32_t* labels, int has_labels) {
  NEED(ctx, "null ctx");
  NEED(feat_type_ok(feat_type), "rau_set_batch_async_packed: feat_type %d (" RAU_FEAT_TYPE_LIST ")", feat_type);
  NEED(counts, "rau_set_batch_async_packed: null counts");
  NEED(n_maps >= 1 && n_maps <= ctx->cfg.B, "rau_set_batch_async_packed: n_maps=%d out of [1,%d]", n_maps, ctx->cfg.B);
  NEED(image_of || n_maps == ctx->cfg.B,
       "rau_set_batch_async_packed: n_maps=%d without image_of (a plain batch has %d maps)", n_maps, ctx->cfg.B);
  return set_batch_slot(ctx, slot, Batch{rows, feat_type, image_of ? n_maps : 0, image_of, tokens, lens, labels,
                                         nullptr, counts},
                        has_labels);
}

int rau_use_batch(rau_ctx* ctx, int slot) {
  NEED(ctx, "null ctx");
  NEED(slot == 0 || slot == 1, "rau_use_batch: slot %d (0 or 1)", slot);
  if (int rc = ensure_async(ctx)) return rc;
  BatchSlot& s = ctx->slot[slot];
  if (!s.held.have) return fail(RAU_ERR_STATE, "rau_use_batch: slot %d holds no batch (rau_set_batch_async)", slot);
  if (slot != ctx->cur_slot) {
    // everything enqueued so far may still read the slot we are leaving (the forward's bulk work is
    // joined into the chain stream by its hop events, the backward's by its end-of-step joins)
    BatchSlot& p = cur_batch(ctx);
    HIPC(hipEventRecord(p.consumed, ctx->st));
    p.consumed_valid = true;
  }
  cur_batch(ctx).held.question = false;   // a question is the resident batch's (rau_set_question_dev): it goes with it
  cur_batch(ctx).held.state = false;      // ... and so is an initial state (rau_set_state_dev)
  cur_batch(ctx).held.att_bias = false;   // ... and an attention bias (rau_set_att_bias_dev)
  ctx->cur_slot = slot;
  drop_forward(ctx);
  s.held.question = false;
  s.held.state = false;
  s.held.att_bias = false;
  // the bulk and weight-gradient streams start each step behind an event of the chain stream,
  // so ordering the chain stream behind the upload orders all three
  HIPC(hipStreamWaitEvent(ctx->st, s.uploaded, 0));
  return RAU_OK;
}

// An answer set for the batch in a slot (slot < 0: the resident batch, synchronous like rau_set_batch; 0 | 1: on
// the copy stream behind the slot's batch, nothing synchronised).  Everything is checked before anything moves.
int rau_set_answers(rau_ctx* ctx, int slot, int32_t G, const int32_t* ids, const float* w, const float* score) {
  NEED(ctx && ids && w, "null argument");
  NEED(slot >= -1 && slot <= 1, "rau_set_answers: slot %d (-1 = the resident batch, 0 or 1)", slot);
  const rau_config& c = ctx->cfg;
  const int si = slot < 0 ? ctx->cur_slot : slot;
  BatchSlot& s = ctx->slot[si];
  if (!s.held.have)
    return fail(RAU_ERR_STATE, "rau_set_answers: slot %d holds no batch (upload the batch first)", si);
  if (slot >= 0 && si == ctx->cur_slot && ctx->fwd.done)
    return fail(RAU_ERR_STATE, "rau_set_answers: slot %d is the current batch of a forward pass whose backward has "
                "not run", si);
  NEED(G >= 1 && G <= kMaxAnswers, "rau_set_answers: G=%d out of [1,%d]", G, kMaxAnswers);
  const size_t n = (size_t)c.B * G;
  for (size_t i = 0; i < n; ++i) {
    NEED(ids[i] >= 0 && ids[i] <= c.K, "rau_set_answers: ids[%zu]=%d out of [0,%d] (0 = empty entry)", i, ids[i], c.K);
    NEED(std::isfinite(w[i]) && w[i] >= 0.f, "rau_set_answers: w[%zu]=%g is negative or not finite", i, (double)w[i]);
    if (score)
      NEED(std::isfinite(score[i]) && score[i] >= 0.f, "rau_set_answers: score[%zu]=%g is negative or not finite", i,
           (double)score[i]);
  }
  if (slot >= 0)
    if (int rc = ensure_async(ctx)) return rc;
  if (int rc = ensure_answers(ctx, si)) return rc;
  if (s.ans_pending) {   // the staging's previous set has not left it yet (two sets for one upload)
    HIPC(hipEventSynchronize(s.uploaded));
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  }
  int32_t* ids_h = s.ans_h;
  float* w_h = reinterpret_cast<float*>(s.ans_h + n);
  float* sc_h = reinterpret_cast<float*>(s.ans_h + 2 * n);
  std::memcpy(ids_h, ids, n * 4);
  std::memcpy(w_h, w, n * 4);
  std::memcpy(sc_h, score ? score : w, n * 4);
  hipStream_t st = slot < 0 ? ctx->st : ctx->stc;
  if (slot < 0) {
    if (s.upload_pending) HIPC(hipStreamWaitEvent(st, s.uploaded, 0));   // behind an asynchronous upload of the batch
  } else {
    // the slot's buffers may still be read by the last step that used them
    if (si == ctx->cur_slot) {
      HIPC(hipEventRecord(s.consumed, ctx->st));
      s.consumed_valid = true;
    }
    if (s.consumed_valid) HIPC(hipStreamWaitEvent(st, s.consumed, 0));
  }
  HIPC(hipMemcpyAsync(s.ans_ids_d, ids_h, n * 4, hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(s.ans_w_d, w_h, n * 4, hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(s.ans_score_d, sc_h, n * 4, hipMemcpyHostToDevice, st));
  if (slot < 0) {
    HIPC(hipStreamSynchronize(st));
    if (s.upload_pending) s.upload_pending = false;   // (the chain stream waited for it above)
  } else {
    HIPC(hipEventRecord(s.uploaded, st));   // rau_use_batch orders the step behind the set too
    s.upload_pending = s.ans_pending = true;
    if (si == ctx->cur_slot) HIPC(hipStreamWaitEvent(ctx->st, s.uploaded, 0));
  }
  s.held.ans_G = G;
  s.held.have_labels = true;   // the set is the batch's ground truth
  if (si == ctx->cur_slot) drop_forward(ctx);
  if (si == ctx->mg.slot) ctx->mg.valid = false;   // statistics of a forward that read the slot's previous targets
  return RAU_OK;
}

int rau_batch_answers(rau_ctx* ctx, int32_t* G) {
  NEED(ctx && G, "null argument");
  *G = truth_of(cur_batch(ctx)).G;
  return RAU_OK;
}

// Region counts for the batch in a slot: rau_set_answers' slot and ordering rules.  Everything is checked before
// anything moves.
int rau_set_regions(rau_ctx* ctx, int slot, const int32_t* n) {
  NEED(ctx && n, "null argument");
  NEED(slot >= -1 && slot <= 1, "rau_set_regions: slot %d (-1 = the resident batch, 0 or 1)", slot);
  const rau_config& c = ctx->cfg;
  const int si = slot < 0 ? ctx->cur_slot : slot;
  BatchSlot& s = ctx->slot[si];
  if (!s.held.have)
    return fail(RAU_ERR_STATE, "rau_set_regions: slot %d holds no batch (upload the batch first)", si);
  if (slot >= 0 && si == ctx->cur_slot && ctx->fwd.done)
    return fail(RAU_ERR_STATE, "rau_set_regions: slot %d is the current batch of a forward pass whose backward has "
                "not run", si);
  for (int b = 0; b < c.B; ++b)
    NEED(n[b] >= 1 && n[b] <= c.S, "rau_set_regions: n[%d]=%d out of [1,%d]", b, n[b], c.S);
  if (slot >= 0)
    if (int rc = ensure_async(ctx)) return rc;
  if (int rc = ensure_regions(ctx, si)) return rc;
  if (s.reg_pending) {   // the staging's previous counts have not left it yet (two sets for one upload)
    HIPC(hipEventSynchronize(s.uploaded));
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  }
  std::memcpy(s.nreg_h, n, (size_t)c.B * 4);
  hipStream_t st = slot < 0 ? ctx->st : ctx->stc;
  if (slot < 0) {
    if (s.upload_pending) HIPC(hipStreamWaitEvent(st, s.uploaded, 0));   // behind an asynchronous upload of the batch
  } else {
    // the slot's buffers may still be read by the last step that used them
    if (si == ctx->cur_slot) {
      HIPC(hipEventRecord(s.consumed, ctx->st));
      s.consumed_valid = true;
    }
    if (s.consumed_valid) HIPC(hipStreamWaitEvent(st, s.consumed, 0));
  }
  HIPC(hipMemcpyAsync(s.nreg_d, s.nreg_h, (size_t)c.B * 4, hipMemcpyHostToDevice, st));
  if (slot < 0) {
    HIPC(hipStreamSynchronize(st));
    // (the chain stream waited for a pending upload above: every copy behind `uploaded` has left its staging)
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  } else {
    HIPC(hipEventRecord(s.uploaded, st));   // rau_use_batch orders the step behind the counts too
    s.upload_pending = s.reg_pending = true;
    if (si == ctx->cur_slot) HIPC(hipStreamWaitEvent(ctx->st, s.uploaded, 0));
  }
  s.held.regions = true;
  if (si == ctx->cur_slot) drop_forward(ctx);   // a forward that ran on the batch did not see these counts
  return RAU_OK;
}

int rau_batch_regions(rau_ctx* ctx, int* has) {
  NEED(ctx && has, "null argument");
  *has = cur_batch(ctx).held.regions ? 1 : 0;
  return RAU_OK;
}

// Attention targets for the batch in a slot: rau_set_regions' slot and ordering rules.  Everything is checked
// before anything moves.  The forward does not read them: its record (rau_ctx::fwd) and the merged-hops record stay.
int rau_set_att_targets(rau_ctx* ctx, int slot, const float* t) {
  NEED(ctx && t, "null argument");
  NEED(slot >= -1 && slot <= 1, "rau_set_att_targets: slot %d (-1 = the resident batch, 0 or 1)", slot);
  const rau_config& c = ctx->cfg;
  const int si = slot < 0 ? ctx->cur_slot : slot;
  BatchSlot& s = ctx->slot[si];
  if (!s.held.have)
    return fail(RAU_ERR_STATE, "rau_set_att_targets: slot %d holds no batch (upload the batch first)", si);
  if (slot >= 0 && si == ctx->cur_slot && ctx->fwd.done)
    return fail(RAU_ERR_STATE, "rau_set_att_targets: slot %d is the current batch of a forward pass whose backward "
                "has not run", si);
  const size_t n = (size_t)c.B * c.S;
  for (size_t i = 0; i < n; ++i)
    NEED(std::isfinite(t[i]) && t[i] >= 0.f, "rau_set_att_targets: t[%zu,%zu]=%g is negative or not finite", i / c.S,
         i % c.S, (double)t[i]);
  if (slot >= 0)
    if (int rc = ensure_async(ctx)) return rc;
  if (int rc = ensure_att_targets(ctx, si)) return rc;
  if (s.att_pending) {   // the staging's previous maps have not left it yet (two sets for one upload)
    HIPC(hipEventSynchronize(s.uploaded));
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  }
  std::memcpy(s.att_t_h, t, n * 4);
  hipStream_t st = slot < 0 ? ctx->st : ctx->stc;
  if (slot < 0) {
    if (s.upload_pending) HIPC(hipStreamWaitEvent(st, s.uploaded, 0));   // behind an asynchronous upload of the batch
  } else {
    // the slot's buffers may still be read by the last step that used them
    if (si == ctx->cur_slot) {
      HIPC(hipEventRecord(s.consumed, ctx->st));
      s.consumed_valid = true;
    }
    if (s.consumed_valid) HIPC(hipStreamWaitEvent(st, s.consumed, 0));
  }
  if (ctx->Sp == c.S)
    HIPC(hipMemcpyAsync(s.att_t_d, s.att_t_h, n * 4, hipMemcpyHostToDevice, st));
  else   // rows of S positions into rows of Sp
    HIPC(hipMemcpy2DAsync(s.att_t_d, (size_t)ctx->Sp * 4, s.att_t_h, (size_t)c.S * 4, (size_t)c.S * 4, c.B,
                          hipMemcpyHostToDevice, st));
  if (slot < 0) {
    HIPC(hipStreamSynchronize(st));
    // (the chain stream waited for a pending upload above: every copy behind `uploaded` has left its staging)
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  } else {
    HIPC(hipEventRecord(s.uploaded, st));   // rau_use_batch orders the step behind the targets too
    s.upload_pending = s.att_pending = true;
    if (si == ctx->cur_slot) HIPC(hipStreamWaitEvent(ctx->st, s.uploaded, 0));
  }
  s.held.att_targets = true;
  return RAU_OK;
}

int rau_batch_att_targets(rau_ctx* ctx, int* has) {
  NEED(ctx && has, "null argument");
  *has = cur_batch(ctx).held.att_targets ? 1 : 0;
  return RAU_OK;
}

// Per-sample loss weights for the batch in a slot: rau_set_regions' slot and ordering rules; NULL detaches them.
// Everything is checked before anything moves.  The forward's head reads them: a forward that ran must run again.
int rau_set_sample_weights(rau_ctx* ctx, int slot, const float* sw) {
  NEED(ctx, "null ctx");
  NEED(slot >= -1 && slot <= 1, "rau_set_sample_weights: slot %d (-1 = the resident batch, 0 or 1)", slot);
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_sample_weights: a step is being captured");
  const rau_config& c = ctx->cfg;
  const int si = slot < 0 ? ctx->cur_slot : slot;
  BatchSlot& s = ctx->slot[si];
  if (!s.held.have)
    return fail(RAU_ERR_STATE, "rau_set_sample_weights: slot %d holds no batch (upload the batch first)", si);
  if (slot >= 0 && si == ctx->cur_slot && ctx->fwd.done)
    return fail(RAU_ERR_STATE, "rau_set_sample_weights: slot %d is the current batch of a forward pass whose backward "
                "has not run", si);
  if (!sw) {   // detach: nothing moves, the next step is the unweighted one
    if (s.held.sample_w && si == ctx->cur_slot) drop_forward(ctx);
    s.held.sample_w = false;
    return RAU_OK;
  }
  for (int b = 0; b < c.B; ++b)
    NEED(std::isfinite(sw[b]) && sw[b] >= 0.f, "rau_set_sample_weights: s[%d]=%g is negative or not finite", b,
         (double)sw[b]);
  if (slot >= 0)
    if (int rc = ensure_async(ctx)) return rc;
  if (int rc = ensure_sample_weights(ctx, si)) return rc;
  if (s.sw_pending) {   // the staging's previous weights have not left it yet (two sets for one upload)
    HIPC(hipEventSynchronize(s.uploaded));
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  }
  std::memcpy(s.sw_h, sw, (size_t)c.B * 4);
  hipStream_t st = slot < 0 ? ctx->st : ctx->stc;
  if (slot < 0) {
    if (s.upload_pending) HIPC(hipStreamWaitEvent(st, s.uploaded, 0));   // behind an asynchronous upload of the batch
  } else {
    // the slot's buffers may still be read by the last step that used them
    if (si == ctx->cur_slot) {
      HIPC(hipEventRecord(s.consumed, ctx->st));
      s.consumed_valid = true;
    }
    if (s.consumed_valid) HIPC(hipStreamWaitEvent(st, s.consumed, 0));
  }
  HIPC(hipMemcpyAsync(s.sw_d, s.sw_h, (size_t)c.B * 4, hipMemcpyHostToDevice, st));
  if (slot < 0) {
    HIPC(hipStreamSynchronize(st));
    // (the chain stream waited for a pending upload above: every copy behind `uploaded` has left its staging)
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  } else {
    HIPC(hipEventRecord(s.uploaded, st));   // rau_use_batch orders the step behind the weights too
    s.upload_pending = s.sw_pending = true;
    if (si == ctx->cur_slot) HIPC(hipStreamWaitEvent(ctx->st, s.uploaded, 0));
  }
  s.held.sample_w = true;
  if (si == ctx->cur_slot) drop_forward(ctx);   // a forward that ran on the batch did not see these weights
  if (si == ctx->mg.slot) ctx->mg.valid = false;   // statistics of a forward whose weights have just been overwritten
  return RAU_OK;
}

int rau_batch_sample_weights(rau_ctx* ctx, int* has) {
  NEED(ctx && has, "null argument");
  *has = cur_batch(ctx).held.sample_w ? 1 : 0;
  return RAU_OK;
}

// Multiple-choice candidates for the batch in a slot: rau_set_answers' slot and ordering rules; NULL or C == 0
// detaches them.  Everything is checked before anything moves.  The forward's head reads them: a forward that ran
// must run again.
int rau_set_candidates(rau_ctx* ctx, int slot, int32_t C, const int32_t* cand) {
  NEED(ctx, "null ctx");
  NEED(slot >= -1 && slot <= 1, "rau_set_candidates: slot %d (-1 = the resident batch, 0 or 1)", slot);
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_candidates: a step is being captured");
  const rau_config& c = ctx->cfg;
  const int si = slot < 0 ? ctx->cur_slot : slot;
  BatchSlot& s = ctx->slot[si];
  if (!s.held.have)
    return fail(RAU_ERR_STATE, "rau_set_candidates: slot %d holds no batch (upload the batch first)", si);
  if (slot >= 0 && si == ctx->cur_slot && ctx->fwd.done)
    return fail(RAU_ERR_STATE, "rau_set_candidates: slot %d is the current batch of a forward pass whose backward has "
                "not run", si);
  if (!cand || C == 0) {   // detach: nothing moves, the next step is the one without candidates
    if (s.held.cand_C > 0) {
      if (si == ctx->cur_slot) drop_forward(ctx);
      if (si == ctx->mg.slot) ctx->mg.valid = false;
    }
    s.held.cand_C = 0;
    return RAU_OK;
  }
  NEED(C >= 1 && C <= kMaxCandidates, "rau_set_candidates: C=%d out of [1,%d]", C, kMaxCandidates);
  const size_t n = (size_t)c.B * C;
  for (size_t i = 0; i < n; ++i)
    NEED(cand[i] >= 0 && cand[i] <= c.K, "rau_set_candidates: cand[%zu]=%d out of [0,%d] (0 = empty entry)", i, cand[i],
         c.K);
  if (slot >= 0)
    if (int rc = ensure_async(ctx)) return rc;
  if (int rc = ensure_candidates(ctx, si)) return rc;
  if (s.cand_pending) {   // the staging's previous list has not left it yet (two lists for one upload)
    HIPC(hipEventSynchronize(s.uploaded));
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  }
  std::memcpy(s.cand_h, cand, n * 4);
  hipStream_t st = slot < 0 ? ctx->st : ctx->stc;
  if (slot < 0) {
    if (s.upload_pending) HIPC(hipStreamWaitEvent(st, s.uploaded, 0));   // behind an asynchronous upload of the batch
  } else {
    // the slot's buffers may still be read by the last step that used them
    if (si == ctx->cur_slot) {
      HIPC(hipEventRecord(s.consumed, ctx->st));
      s.consumed_valid = true;
    }
    if (s.consumed_valid) HIPC(hipStreamWaitEvent(st, s.consumed, 0));
  }
  HIPC(hipMemcpyAsync(s.cand_d, s.cand_h, n * 4, hipMemcpyHostToDevice, st));
  if (slot < 0) {
    HIPC(hipStreamSynchronize(st));
    // (the chain stream waited for a pending upload above: every copy behind `uploaded` has left its staging)
    s.upload_pending = s.ans_pending = s.reg_pending = s.att_pending = s.sw_pending = s.cand_pending = false;
  } else {
    HIPC(hipEventRecord(s.uploaded, st));   // rau_use_batch orders the step behind the list too
    s.upload_pending = s.cand_pending = true;
    if (si == ctx->cur_slot) HIPC(hipStreamWaitEvent(ctx->st, s.uploaded, 0));
  }
  s.held.cand_C = C;
  if (si == ctx->cur_slot) drop_forward(ctx);   // a forward that ran on the batch did not see this list
  if (si == ctx->mg.slot) ctx->mg.valid = false;   // statistics of a forward whose list has just been overwritten
  return RAU_OK;
}

int rau_batch_candidates(rau_ctx* ctx, int32_t* C) {
  NEED(ctx && C, "null argument");
  *C = cur_batch(ctx).held.cand_C;
  return RAU_OK;
}

// The caller's question state for the resident batch: one copy (f32) or exact widening (16-bit) on the chain stream
// into the slot's q_ext, behind every launch that reads the previous contents; nothing waits for the device.  The
// flag is the batch's (BatchDesc::question): the step path branches on it, the graph key carries it.  Everything is
// checked before anything moves.
int rau_set_question_dev(rau_ctx* ctx, const void* q_dev, int q_type) {
  NEED(ctx, "null ctx");
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_question_dev: a step is being captured");
  BatchSlot& s = cur_batch(ctx);
  if (!s.held.have)
    return fail(RAU_ERR_STATE, "rau_set_question_dev: no resident batch (upload the batch first)");
  if (!q_dev) {   // detach: the next step runs the built-in encoder on the batch's tokens
    if (s.held.question) drop_forward(ctx);   // a forward that read the question is not this batch's any more
    s.held.question = false;
    return RAU_OK;
  }
  NEED(q_type == RAU_FEAT_F32 || q_type == RAU_FEAT_F16 || q_type == RAU_FEAT_BF16,
       "rau_set_question_dev: q_type %d is none of RAU_FEAT_F32, RAU_FEAT_F16, RAU_FEAT_BF16", q_type);
  NEED((reinterpret_cast<uintptr_t>(q_dev) & 15u) == 0, "rau_set_question_dev: q_dev must be 16-byte aligned");
  const size_t n = (size_t)ctx->cfg.B, Q = (size_t)ctx->Q;
  if (!s.q_ext)   // for the capacity, at the slot's first question; cleared by rau_set_batch_size like every activation
    if (int rc = dalloc(ctx, &s.q_ext, (size_t)ctx->cap * Q)) return rc;
  hipStream_t st = ctx->st;
  if (q_type == RAU_FEAT_F32)
    HIPC(hipMemcpyAsync(s.q_ext, q_dev, n * Q * sizeof(float), hipMemcpyDeviceToDevice, st));
  else   // Q = 4 Rq elements per row, rows dense: the unpitched path, 4 elements per thread
    RUN("widen_features", 0, (double)n * Q * (4 + feat_elem_bytes(q_type)),
        widen_features(st, n, (int)Q, (int)Q, q_dev, s.q_ext, q_type));
  s.held.question = true;
  drop_forward(ctx);   // a forward that ran on the batch did not read this question
  return RAU_OK;
}

int rau_batch_question(rau_ctx* ctx, int* has) {
  NEED(ctx && has, "null argument");
  *has = cur_batch(ctx).held.question ? 1 : 0;
  return RAU_OK;
}

static int question_grad_state(rau_ctx* ctx, const char* fn) {
  if (!ctx->bwd.dq)
    return fail(RAU_ERR_STATE, "%s: no backward on an attached question (rau_set_question_dev) has run since the "
                "last forward", fn);
  return RAU_OK;
}
int rau_question_grad_dev(rau_ctx* ctx, const float** dq) {
  NEED(ctx, "null ctx");
  if (int rc = question_grad_state(ctx, "rau_question_grad_dev")) return rc;
  if (dq) *dq = ctx->dq;
  return RAU_OK;
}
int rau_get_question_grad(rau_ctx* ctx, float* host) {
  NEED(ctx && host, "null argument");
  if (int rc = question_grad_state(ctx, "rau_get_question_grad")) return rc;
  return d2h(ctx, host, ctx->dq, (size_t)ctx->cfg.B * ctx->Q * sizeof(float));
}

// The caller's additive attention bias for the resident batch: one launch on the chain stream that copies (f32) or
// widens exactly (16-bit) the dense rows [n][S] into the slot's zb_ext at the attention's pitch, behind every launch
// that reads the previous contents; nothing waits for the device.  The flag is the batch's (BatchDesc::att_bias): the
// hop chain hands the buffer to its attention kernels, the backward ends with the gradient's launch, the graph key
// carries it.  Everything is checked before anything moves.
int rau_set_att_bias_dev(rau_ctx* ctx, const void* bias_dev, int type) {
  NEED(ctx, "null ctx");
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_att_bias_dev: a step is being captured");
  BatchSlot& s = cur_batch(ctx);
  if (!s.held.have)
    return fail(RAU_ERR_STATE, "rau_set_att_bias_dev: no resident batch (upload the batch first)");
  if (!bias_dev) {   // detach: the next step's attention kernels get a null pointer again
    if (s.held.att_bias) drop_forward(ctx);   // a forward that read the bias is not this batch's any more
    s.held.att_bias = false;
    ctx->bwd.dbias = false;   // ... nor is the gradient a backward left at it
    return RAU_OK;
  }
  NEED(type == RAU_FEAT_F32 || type == RAU_FEAT_F16 || type == RAU_FEAT_BF16,
       "rau_set_att_bias_dev: type %d is none of RAU_FEAT_F32, RAU_FEAT_F16, RAU_FEAT_BF16", type);
  NEED((reinterpret_cast<uintptr_t>(bias_dev) & 15u) == 0, "rau_set_att_bias_dev: bias_dev must be 16-byte aligned");
  const int n = ctx->cfg.B, SL = ctx->cfg.S, Sp = ctx->Sp;
  // for the capacity, at the first attach; cleared by rau_set_batch_size like every activation
  if (!s.zb_ext)
    if (int rc = dalloc(ctx, &s.zb_ext, (size_t)ctx->cap * Sp)) return rc;
  if (!ctx->zbgrad)
    if (int rc = dalloc(ctx, &ctx->zbgrad, (size_t)ctx->cap * Sp)) return rc;
  RUN("att_bias_attach", 0, (double)n * SL * (4 + feat_elem_bytes(type)),
      att_bias_attach(ctx->st, n, SL, Sp, bias_dev, type, s.zb_ext));
  s.held.att_bias = true;
  ctx->bwd.dbias = false;   // what an earlier backward left is the gradient at ANOTHER bias (or batch)
  drop_forward(ctx);   // a forward that ran on the batch did not read this bias
  return RAU_OK;
}

int rau_batch_att_bias(rau_ctx* ctx, int* has) {
  NEED(ctx && has, "null argument");
  *has = cur_batch(ctx).held.att_bias ? 1 : 0;
  return RAU_OK;
}

static int att_bias_grad_state(rau_ctx* ctx, const char* fn) {
  if (!cur_batch(ctx).held.att_bias || !ctx->bwd.dbias)
    return fail(RAU_ERR_STATE, "%s: no backward on an attached attention bias (rau_set_att_bias_dev) has run since "
                "the last forward", fn);
  return RAU_OK;
}
int rau_att_bias_grad_dev(rau_ctx* ctx, const float** d_bias, int32_t* pitch) {
  NEED(ctx, "null ctx");
  if (int rc = att_bias_grad_state(ctx, "rau_att_bias_grad_dev")) return rc;
  if (d_bias) *d_bias = ctx->zbgrad;
  if (pitch) *pitch = ctx->Sp;
  return RAU_OK;
}
int rau_get_att_bias_grad(rau_ctx* ctx, float* host) {
  NEED(ctx && host, "null argument");
  if (int rc = att_bias_grad_state(ctx, "rau_get_att_bias_grad")) return rc;
  const size_t SL = (size_t)ctx->cfg.S, Sp = (size_t)ctx->Sp;
  if (SL == Sp) return d2h(ctx, host, ctx->zbgrad, (size_t)ctx->cfg.B * SL * sizeof(float));
  HIPC(hipMemcpy2DAsync(host, SL * sizeof(float), ctx->zbgrad, Sp * sizeof(float), SL * sizeof(float),
                        (size_t)ctx->cfg.B, hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);   // d2h's check: never hand back such results as OK
}

// The caller's initial state of the hop chain for the resident batch: one launch on the chain stream that widens
// (c0, h0) into slot 0 of cc / hh, behind every launch that reads the previous contents; nothing waits for the
// device.  The flag is the batch's (BatchDesc::state): the forward leaves the rows alone, the backward hands out the
// gradient at them, the graph key carries it.  Everything is checked before anything moves.
int rau_set_state_dev(rau_ctx* ctx, const void* c0_dev, const void* h0_dev, int type) {
  NEED(ctx, "null ctx");
  if (ctx->capturing) return fail(RAU_ERR_STATE, "rau_set_state_dev: a step is being captured");
  BatchSlot& s = cur_batch(ctx);
  if (!s.held.have)
    return fail(RAU_ERR_STATE, "rau_set_state_dev: no resident batch (upload the batch first)");
  NEED((c0_dev == nullptr) == (h0_dev == nullptr), "rau_set_state_dev: c0 and h0 go together (both NULL = detach)");
  const size_t nR = (size_t)ctx->cfg.B * ctx->cfg.R;
  if (!c0_dev) {   // detach: the zeros of a fresh context are back in the rows before anything reads them
    if (!s.held.state) return RAU_OK;
    RUN("state_attach", 0, (double)nR * 8, state_attach(ctx->st, nR, nullptr, nullptr, RAU_FEAT_F32, ctx->cc, ctx->hh));
    s.held.state = false;
    ctx->bwd.dstate = false;   // ... nor is the gradient a backward left at it
    drop_forward(ctx);   // a forward that read the state is not this batch's any more
    return RAU_OK;
  }
  NEED(type == RAU_FEAT_F32 || type == RAU_FEAT_F16 || type == RAU_FEAT_BF16,
       "rau_set_state_dev: type %d is none of RAU_FEAT_F32, RAU_FEAT_F16, RAU_FEAT_BF16", type);
  NEED(((reinterpret_cast<uintptr_t>(c0_dev) | reinterpret_cast<uintptr_t>(h0_dev)) & 15u) == 0,
       "rau_set_state_dev: c0_dev and h0_dev must be 16-byte aligned");
  if (!ctx->sgrad)   // for the capacity, at the first attach; cleared by rau_set_batch_size like every activation
    if (int rc = dalloc(ctx, &ctx->sgrad, (size_t)2 * ctx->cap * ctx->cfg.R)) return rc;
  RUN("state_attach", 0, (double)nR * 2 * (4 + feat_elem_bytes(type)),
      state_attach(ctx->st, nR, c0_dev, h0_dev, type, ctx->cc, ctx->hh));
  s.held.state = true;
  ctx->bwd.dstate = false;   // what an earlier backward left is the gradient at ANOTHER state (or batch)
  drop_forward(ctx);   // a forward that ran on the batch did not read this state
  return RAU_OK;
}

int rau_batch_state(rau_ctx* ctx, int* has) {
  NEED(ctx && has, "null argument");
  *has = cur_batch(ctx).held.state ? 1 : 0;
  return RAU_OK;
}

static int state_grad_state(rau_ctx* ctx, const char* fn) {
  if (!cur_batch(ctx).held.state || !ctx->bwd.dstate)
    return fail(RAU_ERR_STATE, "%s: no backward on an attached initial state (rau_set_state_dev) has run since the "
                "last forward", fn);
  return RAU_OK;
}
int rau_state_grad_dev(rau_ctx* ctx, const float** d_c0, const float** d_h0) {
  NEED(ctx, "null ctx");
  if (int rc = state_grad_state(ctx, "rau_state_grad_dev")) return rc;
  if (d_c0) *d_c0 = ctx->sgrad;
  if (d_h0) *d_h0 = ctx->sgrad + (size_t)ctx->cap * ctx->cfg.R;
  return RAU_OK;
}
int rau_get_state_grad(rau_ctx* ctx, float* d_c0_host, float* d_h0_host) {
  NEED(ctx, "null ctx");
  if (int rc = state_grad_state(ctx, "rau_get_state_grad")) return rc;
  const size_t nR = (size_t)ctx->cfg.B * ctx->cfg.R;
  if (d_c0_host)
    if (int rc = d2h(ctx, d_c0_host, ctx->sgrad, nR * sizeof(float))) return rc;
  if (d_h0_host)
    if (int rc = d2h(ctx, d_h0_host, ctx->sgrad + (size_t)ctx->cap * ctx->cfg.R, nR * sizeof(float))) return rc;
  return RAU_OK;
}

int rau_batch_feats(rau_ctx* ctx, float** feats_dev) {
  NEED(ctx && feats_dev, "null argument");
  *feats_dev = cur_batch(ctx).feats;
  return RAU_OK;
}

int rau_batch_feat_type(rau_ctx* ctx, int* feat_type) {
  NEED(ctx && feat_type, "null argument");
  *feat_type = cur_batch(ctx).held.feat_type;
  return RAU_OK;
}

int rau_batch_images(rau_ctx* ctx, int* n_images) {
  NEED(ctx && n_images, "null argument");
  *n_images = cur_batch(ctx).held.n_images;
  return RAU_OK;
}

// ------------------------------------------------------------------ feature bank
int rau_bank_create(rau_ctx* ctx, int32_t capacity, int feat_type) {
  NEED(ctx, "null ctx");
  NEED(feat_type_ok(feat_type), "rau_bank_create: feat_type %d (" RAU_FEAT_TYPE_LIST ")", feat_type);
  NEED(capacity >= 1, "rau_bank_create: capacity %d", capacity);
  if (ctx->bank) return fail(RAU_ERR_STATE, "rau_bank_create: the context already has a bank (rau_bank_destroy first)");
  const size_t bytes = (size_t)capacity * ctx->cfg.D * ctx->Sp * feat_elem_bytes(feat_type);
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();   // the failed allocation is reported here, not by the next launch
    return fail(RAU_ERR_NOMEM, "rau_bank_create: hipMalloc(%zu bytes for %d maps) failed: %s", bytes, capacity,
                hipGetErrorString(e));
  }
  e = hipMemsetAsync(d, 0, bytes, ctx->st);   // pad columns stay zero for the bank's lifetime
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->st);
  if (e != hipSuccess) {
    hipFree(d);
    return fail(RAU_ERR_DEVICE, "rau_bank_create: clearing the bank: %s", hipGetErrorString(e));
  }
  ctx->bank = d;
  ctx->bank_cap = capacity;
  ctx->bank_type = feat_type;
  ctx->bank_filled = 0;
  ctx->bank_written.assign((size_t)capacity, 0);
  return RAU_OK;
}

int rau_bank_destroy(rau_ctx* ctx) {
  NEED(ctx, "null ctx");
  if (!ctx->bank) return RAU_OK;
  if (int rc = bank_quiesce(ctx)) return rc;
  // captured steps of bank batches hold the bank's address
  for (auto it = ctx->graphs.begin(); it != ctx->graphs.end();)
    if (it->key.bank) { hipGraphExecDestroy(it->exec); it = ctx->graphs.erase(it); } else ++it;
  for (BatchSlot& s : ctx->slot) {   // a batch drawn from the bank is gone with it
    if (!s.held.bank) continue;
    const int ft = s.held.feat_type;   // (its maps are not: enqueue_batch's pad-column rule reads their type)
    s.held = BatchDesc{};
    s.held.feat_type = ft;
    if (&s == &cur_batch(ctx)) drop_forward(ctx);
  }
  hipFree(ctx->bank);
  if (ctx->bank_stage) hipFree(ctx->bank_stage);
  if (ctx->bank_meta_d) hipFree(ctx->bank_meta_d);
  ctx->bank_meta_d = nullptr;
  for (int k = 0; k < 2; ++k) {
    if (ctx->bank_pin[k]) hipHostFree(ctx->bank_pin[k]);
    if (ctx->bank_ev[k]) hipEventDestroy(ctx->bank_ev[k]);
    if (ctx->bank_meta_pin[k]) hipHostFree(ctx->bank_meta_pin[k]);
    ctx->bank_pin[k] = nullptr;
    ctx->bank_ev[k] = nullptr;
    ctx->bank_meta_pin[k] = nullptr;
  }
  ctx->bank = nullptr;
  ctx->bank_stage = nullptr;
  ctx->bank_chunk = 0;
  ctx->bank_cap = ctx->bank_filled = 0;
  ctx->bank_written.clear();
  ctx->x_valid = false;
  return RAU_OK;
}

int rau_bank_info(rau_ctx* ctx, int32_t* capacity, int* feat_type, int32_t* rows_filled) {
  NEED(ctx, "null ctx");
  if (!ctx->bank) return fail(RAU_ERR_STATE, "rau_bank_info: the context has no feature bank");
  if (capacity) *capacity = ctx->bank_cap;
  if (feat_type) *feat_type = ctx->bank_type;
  if (rows_filled) *rows_filled = ctx->bank_filled;
  return RAU_OK;
}

int rau_bank_put(rau_ctx* ctx, int32_t first, int32_t count, const void* feats, int src_type) {
  NEED(ctx && feats, "null argument");
  if (!ctx->bank) return fail(RAU_ERR_STATE, "rau_bank_put: the context has no feature bank (rau_bank_create)");
  NEED(feat_type_ok(src_type), "rau_bank_put: src_type %d (" RAU_FEAT_TYPE_LIST ")", src_type);
  NEED(src_type == ctx->bank_type || src_type == RAU_FEAT_F32,
       "rau_bank_put: maps of type %d into a bank of type %d (equal types, or f32 into a 16-bit or fp8 bank)", src_type,
       ctx->bank_type);
  NEED(first >= 0 && count >= 1 && (int64_t)first + count <= ctx->bank_cap, "rau_bank_put: rows [%d,%d) out of [0,%d)",
       first, first + count, ctx->bank_cap);
  const rau_config& c = ctx->cfg;
  const bool narrow = src_type != ctx->bank_type;
  const size_t ses = feat_elem_bytes(src_type), src_map = (size_t)c.D * c.S * ses, map_bytes = bank_map_bytes(ctx);
  const size_t bes = feat_elem_bytes(ctx->bank_type);
  if (int rc = ensure_bank_staging(ctx, narrow)) return rc;
  if (int rc = bank_quiesce(ctx)) return rc;   // enqueued gathers read the rows being replaced
  const int32_t per = (int32_t)std::min<size_t>(ctx->bank_chunk / src_map, (size_t)count);
  hipStream_t st = ctx->st;
  bool used[2] = {false, false};
  int k = 0;
  for (int32_t r0 = 0; r0 < count; r0 += per, k ^= 1) {
    const int32_t n = std::min(per, count - r0);
    if (used[k]) HIPC(hipEventSynchronize(ctx->bank_ev[k]));   // the staging's last copy has left it
    std::memcpy(ctx->bank_pin[k], static_cast<const char*>(feats) + (size_t)r0 * src_map, (size_t)n * src_map);
    char* dst = static_cast<char*>(ctx->bank) + (size_t)(first + r0) * map_bytes;
    if (narrow) {
      // (one device staging: the stream orders the next chunk's copy behind this chunk's kernel)
      HIPC(hipMemcpyAsync(ctx->bank_stage, ctx->bank_pin[k], (size_t)n * src_map, hipMemcpyHostToDevice, st));
      RUN("bank_narrow", 0, (double)n * (src_map + map_bytes),
          narrow_features(st, (size_t)n * c.D, c.S, ctx->Sp, ctx->bank_stage, dst, ctx->bank_type));
    } else if (ctx->Sp == c.S) {
      HIPC(hipMemcpyAsync(dst, ctx->bank_pin[k], (size_t)n * src_map, hipMemcpyHostToDevice, st));
    } else {
      HIPC(hipMemcpy2DAsync(dst, (size_t)ctx->Sp * bes, ctx->bank_pin[k], (size_t)c.S * bes, (size_t)c.S * bes,
                            (size_t)n * c.D, hipMemcpyHostToDevice, st));
    }
    HIPC(hipEventRecord(ctx->bank_ev[k], st));
    used[k] = true;
  }
  HIPC(hipStreamSynchronize(st));
  for (int32_t r = first; r < first + count; ++r)
    if (!ctx->bank_written[r]) { ctx->bank_written[r] = 1; ++ctx->bank_filled; }
  ctx->x_valid = false;   // an expansion made from replaced rows is stale
  return RAU_OK;
}

// rau_bank_put for packed region rows: map first + i owns counts[i] rows of `rows`.  Chunks of whole maps go
// through the pinned staging into the device staging, and unpack_regions writes them into the bank's rows, dense
// and zero behind each count (narrowing f32 on the way where the bank is narrower).
int rau_bank_put_packed(rau_ctx* ctx, int32_t first, int32_t count, const void* rows, int src_type,
                        const int32_t* counts) {
  NEED(ctx && rows && counts, "null argument");
  if (!ctx->bank) return fail(RAU_ERR_STATE, "rau_bank_put_packed: the context has no feature bank (rau_bank_create)");
  NEED(feat_type_ok(src_type), "rau_bank_put_packed: src_type %d (" RAU_FEAT_TYPE_LIST ")", src_type);
  NEED(src_type == ctx->bank_type || src_type == RAU_FEAT_F32,
       "rau_bank_put_packed: rows of type %d into a bank of type %d (equal types, or f32 into a 16-bit or fp8 bank)",
       src_type, ctx->bank_type);
  NEED(first >= 0 && count >= 1 && (int64_t)first + count <= ctx->bank_cap,
       "rau_bank_put_packed: rows [%d,%d) out of [0,%d)", first, first + count, ctx->bank_cap);
  const rau_config& c = ctx->cfg;
  for (int32_t i = 0; i < count; ++i)
    NEED(counts[i] >= 1 && counts[i] <= c.S, "rau_bank_put_packed: counts[%d]=%d out of [1,%d]", i, counts[i], c.S);
  if (int rc = ensure_bank_staging(ctx, true)) return rc;
  for (int k = 0; k < 2; ++k)
    if (!ctx->bank_meta_pin[k]) {
      void* h = nullptr;
      hipError_t e = hipHostMalloc(&h, 2 * (size_t)kBankPackMaps * 4, hipHostMallocDefault);
      if (e != hipSuccess)
        return fail(RAU_ERR_NOMEM, "rau_bank_put_packed: hipHostMalloc(offsets staging): %s", hipGetErrorString(e));
      ctx->bank_meta_pin[k] = static_cast<int32_t*>(h);
    }
  if (!ctx->bank_meta_d) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&ctx->bank_meta_d), 2 * (size_t)kBankPackMaps * 4);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      ctx->bank_meta_d = nullptr;
      return fail(RAU_ERR_NOMEM, "rau_bank_put_packed: hipMalloc(offsets): %s", hipGetErrorString(e));
    }
  }
  if (int rc = bank_quiesce(ctx)) return rc;   // enqueued gathers read the rows being replaced
  const size_t row_bytes = (size_t)c.D * feat_elem_bytes(src_type), map_bytes = bank_map_bytes(ctx);
  const size_t chunk_rows = ctx->bank_chunk / row_bytes;   // >= S: the staging holds at least one f32 map
  hipStream_t st = ctx->st;
  bool used[2] = {false, false};
  int k = 0;
  const char* src = static_cast<const char*>(rows);
  for (int32_t i0 = 0; i0 < count; k ^= 1) {
    if (used[k]) HIPC(hipEventSynchronize(ctx->bank_ev[k]));   // the staging's last copies have left it
    int32_t* meta = ctx->bank_meta_pin[k];
    int32_t n = 0;
    size_t nrows = 0;
    while (i0 + n < count && n < kBankPackMaps && nrows + (size_t)counts[i0 + n] <= chunk_rows) {
      meta[n] = (int32_t)nrows;
      nrows += (size_t)counts[i0 + n];
      ++n;
    }
    for (int32_t i = 0; i < n; ++i) meta[n + i] = counts[i0 + i];
    std::memcpy(ctx->bank_pin[k], src, nrows * row_bytes);
    char* dst = static_cast<char*>(ctx->bank) + (size_t)(first + i0) * map_bytes;
    // (one device staging: the stream orders the next chunk's copies behind this chunk's kernel)
    HIPC(hipMemcpyAsync(ctx->bank_stage, ctx->bank_pin[k], nrows * row_bytes, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(ctx->bank_meta_d, meta, 2 * (size_t)n * 4, hipMemcpyHostToDevice, st));
    RUN("unpack_regions", 0, (double)(nrows * row_bytes + (size_t)n * map_bytes),
        unpack_regions(st, n, c.D, c.S, ctx->Sp, ctx->bank_stage, nrows, ctx->bank_meta_d, ctx->bank_meta_d + n, dst,
                       src_type, ctx->bank_type));
    HIPC(hipEventRecord(ctx->bank_ev[k], st));
    used[k] = true;
    src += nrows * row_bytes;
    i0 += n;
  }
  HIPC(hipStreamSynchronize(st));
  for (int32_t r = first; r < first + count; ++r)
    if (!ctx->bank_written[r]) { ctx->bank_written[r] = 1; ++ctx->bank_filled; }
  ctx->x_valid = false;   // an expansion made from replaced rows is stale
  return RAU_OK;
}

int rau_bank_get(rau_ctx* ctx, int32_t first, int32_t count, void* feats) {
  NEED(ctx && feats, "null argument");
  if (!ctx->bank) return fail(RAU_ERR_STATE, "rau_bank_get: the context has no feature bank (rau_bank_create)");
  NEED(first >= 0 && count >= 1 && (int64_t)first + count <= ctx->bank_cap, "rau_bank_get: rows [%d,%d) out of [0,%d)",
       first, first + count, ctx->bank_cap);
  const rau_config& c = ctx->cfg;
  const size_t bes = feat_elem_bytes(ctx->bank_type), map_bytes = bank_map_bytes(ctx);
  const char* src = static_cast<const char*>(ctx->bank) + (size_t)first * map_bytes;
  HIPC(hipStreamSynchronize(ctx->st));
  if (ctx->Sp == c.S)
    HIPC(hipMemcpy(feats, src, (size_t)count * map_bytes, hipMemcpyDeviceToHost));
  else
    HIPC(hipMemcpy2D(feats, (size_t)c.S * bes, src, (size_t)ctx->Sp * bes, (size_t)c.S * bes, (size_t)count * c.D,
                     hipMemcpyDeviceToHost));
  return RAU_OK;
}

}  // extern "C"

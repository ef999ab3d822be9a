// bmx_first.inc — the first node per group (bmx_first.h): bmx_where_group_first and its sharded form. The program, the width dispatch of the sweep and the entry
// guards are bmx_where.inc's (where_prepare, where_sweep, where_enter, where_comm_guard), the table, its scratch and the grouped-answer steps bmx_group.inc's
// (group_scratch, group_slots, group_finish_grid, grouped_collect, comm_grouped), the kernels first_kernels.h. The context keeps what the form adds to
// GroupScratch (FirstScratch): one id word per slot, which every query's last kernel leaves at BMX_FIRST_NO_NODE again (clean), the words per index position
// that pass 1 leaves pass 2 (allocated by the first query, grown with the index) and the staging of a host-mode answer. Passes 1 and 2 are a step of their own
// (first_passes), which bmx_group_top.inc enqueues too. Included by bmx.hip (one translation unit), behind everything that was here before it.
namespace {

struct FirstWant { uint32_t group_field, order_field, nfields; const uint32_t* fields; uint32_t flags; uint64_t cap; };
inline uint32_t first_cols(const FirstWant& w) { return w.nfields * ((w.flags & BMX_ROWS_TS) ? 2u : 1u); }     // columns of 8-byte cells beside the records

const char* first_bad_args(const FirstWant& w, const bmx_first_rec* out, const int64_t* out_val, const int64_t* out_ts, const bmx_first_res* res) {
  if (!res) return "bmx_where_group_first: null result record";
  if (w.cap == 0 || w.cap > BMX_FIRST_MAX_CAP) return "bmx_where_group_first: cap outside 1..BMX_FIRST_MAX_CAP";
  if (!out) return "bmx_where_group_first: null output";
  if (w.nfields > BMX_ROWS_MAX_FIELDS) return "bmx_where_group_first: more than BMX_ROWS_MAX_FIELDS fields";
  if (w.nfields && !w.fields) return "bmx_where_group_first: null fields";
  if (w.nfields && !out_val) return "bmx_where_group_first: null out_val";
  if (w.nfields && (w.flags & BMX_ROWS_TS) && !out_ts) return "bmx_where_group_first: null out_ts";
  if (w.flags & ~(BMX_ROWS_TS | BMX_FIRST_DESC)) return "bmx_where_group_first: unknown flag bits in flags";
  if (w.group_field == BMX_AGG_NO_FIELD) return "bmx_where_group_first: no group field";
  if (w.order_field == BMX_AGG_NO_FIELD) return "bmx_where_group_first: no order field";
  return nullptr;
}

// the form's own scratch for a table of `slots` slots over an index of n positions (group_scratch has sized and cleaned the table itself)
int first_scratch(bmx_ctx* ctx, uint64_t slots, uint64_t n) {
  FirstScratch& s = ctx->first;
  if (slots > s.slots) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.slots = 0;
    if (int rc = dev_alloc_all(ctx, {{s.idw, slots * sizeof(unsigned long long)}})) return rc;
    s.slots = slots; s.clean = false;
  }
  if (!s.clean) {
    hipLaunchKernelGGL(k_first_clear, dim3(group_finish_grid(s.slots)), dim3(256), 0, ctx->stream, s.idw, s.slots);
    LAUNCHCHK("k_first_clear");
    s.clean = true;
  }
  if (n > s.pos_cap || !s.gw) {       // (whole units of the sweep: a lane stores its unit's words as vectors)
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.pos_cap = 0;
    const uint64_t cap = (std::max<uint64_t>(n, 1) + n / 4 + 15) & ~15ull;
    if (int rc = dev_alloc_all(ctx, {{s.gw, cap * sizeof(long long)}, {s.ow, cap * sizeof(long long)}})) return rc;
    s.pos_cap = cap;
  }
  return BMX_OK;
}

// room for the staged records, `words` 8-byte words of staged columns and the result record
int first_stage(bmx_ctx* ctx, uint64_t cap, uint64_t words) {
  FirstScratch& s = ctx->first;
  words = std::max<uint64_t>(words, 1);
  if (cap > s.stage_cap || words > s.stage_words) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    cap = std::max(cap, s.stage_cap); words = std::max(words, s.stage_words);
    s.stage_cap = 0; s.stage_words = 0;
    if (int rc = dev_alloc_all(ctx, {{s.stage, cap * sizeof(bmx_first_rec)}, {s.stage_cols, words * 8}, {s.stage_res, sizeof(bmx_first_res)}})) return rc;
    s.stage_cap = cap; s.stage_words = words;
  }
  return BMX_OK;
}

// Passes 1 and 2 of one query over a prepared program (k_first_sweep, k_first_resolve): the table, the words per position and, per key that has a contender,
// the smallest id on its extreme in the id word. F gets what the kernels behind them need. Both scratches are marked unclean; the caller marks them clean behind
// its last kernel. The arguments have been checked and the context entered. A value-ordered view of the base field's index is neither read nor touched
// (where_run).
int first_passes(bmx_ctx* ctx, Index* ix, uint32_t base_field, const WhereProg& W, uint32_t group_field, uint32_t order_field, bool desc, uint64_t cap, FirstArgs& F) {
  if (int rc = group_scratch(ctx, cap)) return rc;
  FirstScratch& s = ctx->first;
  F = FirstArgs{};
  GroupArgs& A = F.G;
  A.keys = ctx->group.keys; A.acc = ctx->group.acc; A.S = ctx->group.state;
  A.slots = group_slots(cap); A.cap = cap;
  if (int rc = first_scratch(ctx, A.slots, ix->n)) return rc;
  A.measure = order_field; A.group = group_field;
  A.m_src = where_agg_source(order_field, base_field); A.g_src = where_agg_source(group_field, base_field);
  F.idw = s.idw;
  F.same = (order_field == group_field && A.g_src == AGG_SRC_PROBE) ? 1u : 0u;
  F.desc = desc ? 1u : 0u;
  F.gw = A.g_src == AGG_SRC_PROBE ? s.gw : nullptr;
  F.ow = ((A.m_src == AGG_SRC_PROBE && !F.same) || !F.gw) ? s.ow : nullptr;
  ctx->group.clean = false; s.clean = false;
  where_sweep_c(ctx, ix, W, [&](const auto& P, uint32_t blocks) {
    hipLaunchKernelGGL((k_first_sweep<decltype(where_value(P)), where_clocks<decltype(P)>>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, ix->n, P, F);
  });
  LAUNCHCHK("k_first_sweep");
  const uint32_t rgrid = sweep_grid(ctx, ix->n, 8ull * FIRST_THREADS);
  by_width(ix->fits32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_first_resolve<T>), dim3(rgrid), dim3(FIRST_THREADS), 0, ctx->stream,
                       sizeof(T) == 4 ? reinterpret_cast<const T*>(ix->v32) : reinterpret_cast<const T*>(ix->v64), ix->ids, ix->n, F);
  });
  LAUNCHCHK("k_first_resolve");
  return BMX_OK;
}

// Enqueue one query over a prepared program; the records, the columns (stride w.cap) and the result record go to d_out / d_val / d_ts / d_res (device memory),
// or, with d_out == nullptr, to the context's staging (first_collect fetches them). The arguments have been checked and the context entered.
int first_enqueue(bmx_ctx* ctx, uint32_t base_field, const WhereProg& W, const FirstWant& w, bmx_first_rec* d_out, int64_t* d_val, int64_t* d_ts, bmx_first_res* d_res) {
  Index* ix;
  if (int rc = fresh_index(ctx, base_field, &ix)) return rc;
  FirstScratch& s = ctx->first;
  if (!d_out) {
    if (int rc = first_stage(ctx, w.cap, w.cap * first_cols(w))) return rc;
    d_out = s.stage; d_res = s.stage_res;
    d_val = reinterpret_cast<int64_t*>(s.stage_cols); d_ts = d_val + (uint64_t)w.nfields * w.cap;
  }
  FirstArgs F;
  if (int rc = first_passes(ctx, ix, base_field, W, w.group_field, w.order_field, (w.flags & BMX_FIRST_DESC) != 0, w.cap, F)) return rc;
  const GroupArgs& A = F.G;
  FirstOut O{};
  O.slots = ctx->slots; O.nslots = ctx->nslots;
  O.out = d_out; O.out_val = d_val; O.out_ts = d_ts; O.res = d_res;
  O.nfields = w.nfields; O.with_ts = (w.flags & BMX_ROWS_TS) ? 1u : 0u;
  for (uint32_t f = 0; f < w.nfields; f++) O.field[f] = w.fields[f];
  hipLaunchKernelGGL(k_first_finish, dim3(group_finish_grid(A.slots)), dim3(256), 0, ctx->stream, F, O, A.m_src != AGG_SRC_PROBE ? 1u : 0u);
  LAUNCHCHK("k_first_finish");
  ctx->group.clean = true; s.clean = true;
  return BMX_OK;
}

inline bool first_key_less(const bmx_first_rec& a, const bmx_first_rec& b) { return a.key < b.key; }

// Second half of a staged answer: the result record, the records sorted by key and their first_cols(w) columns, rows moved with the records, packed with
// stride recs.size() into `cols`. Nothing of the caller's is written.
int first_collect(bmx_ctx* ctx, const FirstWant& w, std::vector<bmx_first_rec>& recs, std::vector<int64_t>& cols, bmx_first_res* res) {
  const FirstScratch& s = ctx->first;
  std::vector<uint32_t> perm;
  if (int rc = grouped_collect(ctx, s.stage, s.stage_res, BMX_FIRST_OVERFLOW, w.cap, first_key_less, "bmx_where_group_first", recs, res, &perm)) return rc;
  const uint64_t m = recs.size(), nc = first_cols(w);
  cols.assign(m * nc, 0);
  if (!m || !nc) return BMX_OK;
  std::vector<int64_t> raw(m * nc);
  for (uint64_t c = 0; c < nc; c++)
    HIPCHK(hipMemcpyAsync(raw.data() + c * m, reinterpret_cast<const int64_t*>(s.stage_cols) + c * w.cap, m * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (uint64_t c = 0; c < nc; c++)
    for (uint64_t i = 0; i < m; i++) cols[c * m + i] = raw[c * m + perm[i]];
  return BMX_OK;
}

// packed columns (stride m) -> the caller's (stride w.cap): the values of the fields, then their clocks
void first_deliver(const FirstWant& w, const std::vector<int64_t>& cols, uint64_t m, int64_t* out_val, int64_t* out_ts) {
  if (!m) return;
  for (uint32_t f = 0; f < w.nfields; f++) {
    std::memcpy(out_val + (uint64_t)f * w.cap, cols.data() + (uint64_t)f * m, m * 8);
    if (w.flags & BMX_ROWS_TS) std::memcpy(out_ts + (uint64_t)f * w.cap, cols.data() + ((uint64_t)w.nfields + f) * m, m * 8);
  }
}

// does record a come before record b under the order (both have a node)?
inline bool first_better(const bmx_first_rec& a, const bmx_first_rec& b, bool desc) {
  if (a.val != b.val) return desc ? a.val > b.val : a.val < b.val;
  return a.id < b.id;
}

// one record of the sharded merge: where its cells are
struct FirstRow { bmx_first_rec r; uint32_t shard, row; };

}  // namespace

extern "C" {

int bmx_where_group_first(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t group_field,
                          uint32_t order_field, uint32_t nfields, const uint32_t* fields, uint32_t flags, uint64_t cap, bmx_first_rec* out, int64_t* out_val,
                          int64_t* out_ts, bmx_first_res* res, int mem) {
  WhereProg W;
  const FirstWant w{group_field, order_field, nfields, fields, flags, cap};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (const char* bad = first_bad_args(w, out, out_val, out_ts, res)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (int erc = where_enter(ctx, mem)) return erc;
  if (mem == BMX_MEM_DEVICE) return first_enqueue(ctx, base_field, W, w, out, out_val, out_ts, res);
  if (int rc = first_enqueue(ctx, base_field, W, w, nullptr, nullptr, nullptr, nullptr)) return rc;
  std::vector<bmx_first_rec> recs;
  std::vector<int64_t> cols;
  bmx_first_res r;
  if (int rc = first_collect(ctx, w, recs, cols, &r)) return rc;
  if (!recs.empty()) std::memcpy(out, recs.data(), recs.size() * sizeof(bmx_first_rec));
  first_deliver(w, cols, recs.size(), out_val, out_ts);
  *res = r;
  return BMX_OK;
}

int bmx_comm_where_group_first(bmx_comm* c, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, uint32_t group_field,
                               uint32_t order_field, uint32_t nfields, const uint32_t* fields, uint32_t flags, uint64_t cap, bmx_first_rec* out, int64_t* out_val,
                               int64_t* out_ts, bmx_first_res* res) {
  WhereProg W;
  const FirstWant w{group_field, order_field, nfields, fields, flags, cap};
  if (const char* bad = where_prepare(base_field, nclauses, clause_len, lits, &W)) return fail(c, BMX_ERR_INVALID, bad);
  if (const char* bad = first_bad_args(w, out, out_val, out_ts, res)) return fail(c, BMX_ERR_INVALID, bad);
  if (int rc = where_comm_guard(c)) return rc;
  DevGuard guard;
  const bool desc = (flags & BMX_FIRST_DESC) != 0;
  const uint32_t nc = first_cols(w);
  std::vector<std::vector<int64_t>> cols;          // per shard, in shard order: its packed columns
  std::vector<uint64_t> rows;                      // ... and their stride
  std::vector<bmx_first_rec> recs;
  std::vector<FirstRow> merged(cap);
  bmx_first_res tot;
  if (int rc = comm_grouped(c, cap, BMX_FIRST_OVERFLOW, [](const FirstRow& a, const FirstRow& b) { return a.r.key < b.r.key; }, merged.data(), &tot,
        [&](bmx_ctx* x) { return first_enqueue(x, base_field, W, w, nullptr, nullptr, nullptr, nullptr); },
        [&](bmx_ctx* x, std::vector<FirstRow>& part, bmx_first_res* r) {
          cols.emplace_back();
          const int crc = first_collect(x, w, recs, cols.back(), r);
          rows.push_back(crc ? 0 : recs.size());
          part.clear();
          if (crc) return crc;
          for (uint32_t i = 0; i < recs.size(); i++) part.push_back(FirstRow{recs[i], (uint32_t)cols.size() - 1u, i});
          return (int)BMX_OK;
        },
        [](uint32_t, bmx_first_res& t, const bmx_first_res& r) { t.total += r.total; t.absent += r.absent; t.n_ordered += r.n_ordered; },
        [&](FirstRow& m, const FirstRow& p) {          // counts add; the better (val, id) wins and brings its shard's cells
          const uint64_t nm = m.r.n_match + p.r.n_match, n = m.r.n + p.r.n;
          if (p.r.n && (!m.r.n || first_better(p.r, m.r, desc))) m = p;
          m.r.n_match = nm; m.r.n = n;
        })) return rc;
  if (!(tot.flags & BMX_FIRST_OVERFLOW)) {
    for (uint64_t i = 0; i < tot.n_groups; i++) {
      const FirstRow& m = merged[i];
      out[i] = m.r;
      for (uint32_t k = 0; k < nc; k++) {
        int64_t* dst = k < nfields ? out_val + (uint64_t)k * cap : out_ts + (uint64_t)(k - nfields) * cap;
        dst[i] = cols[m.shard][(uint64_t)k * rows[m.shard] + m.row];
      }
    }
  }
  *res = tot;
  return BMX_OK;
}

}  // extern "C"
